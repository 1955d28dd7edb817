"""The fast AR of ar_decode_kernel (ar_decode.hip) where it leaves the generic phase sequence:
  * layer 0 of codebooks 1..7 reads row `token` of the engine's table fast_qkv0 (RMSNorm + wqkv of every fast_embeddings row, filled once
    by the kernel's own fill mode) in place of phase FA and its all-gather;
  * codebook 0 attends to one key, so its attention output is V;
  * codebooks 1..7 hold one head per 16-lane row and normalise in registers (tests/test_fast_attention_order_cpu.py has the order).

Table rows are compared bit for bit with ardev::gemv<WT, 768, 6, 1, true> through its test hook (engine.test_ar_gemv), in both AR element
types.  Whole frames are compared with the float64 frame of tests/ar_frame_ref.py under the bound tests/test_gpu_ar_frame.py states (its own
_check_frame), from the engine's own state, on the smallest shapes: 3-frame prompts, chunk_frames = 1, one and two slots in one launch.  The
teacher-forced codes choose the table rows: all 0, all 999 (the last row), eight distinct codes, and one code everywhere but the middle
(equal keys: a flat softmax over up to 8 positions).  One more frame is unforced with host noise, and two slots with identical state and
noise must agree bit for bit."""
import numpy as np
import pytest
import torch

import ar_frame_ref as R
import test_gpu_ar_frame as T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

M = "arvc.decoder.model."
V, NCB, CBS, D = 8192, 8, 1000, 768


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


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_table_rows_are_phase_fa_bits(engines, weights0, half):
    from streamvoiceanon_amd import engine as E
    eng = engines(half)
    wqkv = weights0[M + "fast_layers.0.attention.wqkv.weight"].numpy()
    nw = weights0[M + "fast_layers.0.attention_norm.weight"].numpy()
    emb = weights0[M + "fast_embeddings.weight"].numpy()
    assert wqkv.shape == (3 * D, D) and emb.shape == (CBS, D)
    rows = [0, 1, CBS - 1] + [int(r) for r in np.random.default_rng(7).integers(2, CBS - 1, 3)]
    for r in rows:
        want, same = E.test_ar_gemv(5, wqkv, emb[r][None], nw, half=half)          # instance 5 = <K 768, ROWS 6, M 1, NORM>
        assert same.all()
        got = eng.fast_qkv0_rows(r)
        assert got.shape == (1, 3 * D) and np.isfinite(got).all()
        assert got.tobytes() == want.tobytes(), (r, float(np.abs(got - want).max()))
    assert eng.fast_qkv0_rows(CBS - 2, 2).tobytes() == np.concatenate([eng.fast_qkv0_rows(CBS - 2), eng.fast_qkv0_rows(CBS - 1)]).tobytes()
    for row0, n in ((-1, 1), (CBS, 1), (CBS - 1, 2), (0, 0)):
        with pytest.raises(RuntimeError, match="sva_test_fast_qkv0"):
            eng.fast_qkv0_rows(row0, n)


def _forced_patterns(rng):
    distinct = rng.choice(CBS, NCB, replace=False)
    same = np.full(NCB, int(rng.integers(0, CBS)))
    same[NCB // 2] = (same[0] + 1 + int(rng.integers(0, CBS - 1))) % CBS
    assert len(set(distinct.tolist())) == NCB and len(set(same.tolist())) == 2
    return [np.zeros(NCB, np.int64), np.full(NCB, CBS - 1), distinct, same]


def _start(b, seeds, rng, fill=None):
    from streamvoiceanon_amd.synth_audio import synth_prompt
    for s, seed in enumerate(seeds):
        ac, cc, style, timbre = synth_prompt(seed, 3)
        b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=seed)
    b.begin()
    b.ar_delay_fill(rng.integers(0, V, (b.B, T.DELAY)) if fill is None else fill)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_forced_and_free_frames_match_fp64(engines, w64s, half, B):
    eng, W64 = engines(half), w64s(half)
    rng = np.random.default_rng(900 + 10 * B + int(half))
    pats = _forced_patterns(rng)
    b = T._make_batch(eng, B, T.MODE_PER_STREAM)
    case = f"fast-path-{'fp16' if half else 'fp32'}-B{B}"
    worst, failures, n_near, n_samp = {}, [], 0, 0
    try:
        assert b.decode_path() == 1
        _start(b, [4000 + 10 * int(half) + s for s in range(B)], rng)
        lp = b.tap("last_pos", (B,), np.int32).copy()
        np.testing.assert_array_equal(lp, [R.last_pos_after_fill(3, T.DELAY)] * B)
        # two frames per pattern (slot s takes pattern p + s, so a two-slot launch carries two patterns at once), then one unforced frame
        plan = [[pats[(p + s) % len(pats)] for s in range(B)] for p in range(len(pats)) for _ in range(2)] + [None]
        for f, forced in enumerate(plan):
            emb = b.tap("cached_audio_emb", (B, D))
            states = [R.state_from_batch(b, s, int(lp[s]), emb[s]) for s in range(B)]
            code = rng.integers(0, V, B)
            noise = (rng.exponential(size=(B, V + NCB * CBS)) + 1e-9).astype(np.float32)
            codes, pos = b.ar_decode_one(code, noise=noise, forced=None if forced is None else np.stack(forced).astype(np.int32))
            assert int(b.tap("ar_fail", (1,), np.int32)[0]) == 0, (case, f)
            np.testing.assert_array_equal(pos, lp + 2)
            fast = b.tap("fast_logits", (B, NCB, CBS))
            slow = b.tap("slow_logits", (B, V))
            hidden = b.tap("hidden", (B, D))
            emb_new = b.tap("cached_audio_emb", (B, D))
            raw = b.tap("sampled_codes", (B, NCB), np.int32)
            assert np.isfinite(fast).all() and np.isfinite(slow).all()
            if forced is not None:
                np.testing.assert_array_equal(codes, np.stack(forced))
            else:
                np.testing.assert_array_equal(codes, raw)
                assert ((codes >= 0) & (codes < CBS)).all()
            for s in range(B):
                for cb in range(NCB):       # the sampler reads this codebook's logits and noise: the engine's own row, in float64
                    tok, near = R.sample_f64(fast[s, cb], noise[s, V + cb * CBS:V + (cb + 1) * CBS], 0.7, 0.7)
                    n_samp += 1
                    n_near += int(near)
                    assert near or tok == int(raw[s, cb]), (case, "sampled code", dict(frame=f, slot=s, codebook=cb, want=tok, got=int(raw[s, cb])))
            for s in range(B):
                new = b.kv_rows(s, int(lp[s]) + 1, 2).astype(np.float64)
                ref = R.frame_fp64(W64, states[s], int(code[s]), codes[s])
                got = dict(slow_logits=slow[s].astype(np.float64), fast_logits=fast[s].astype(np.float64), hidden=hidden[s].astype(np.float64),
                           emb=emb_new[s].astype(np.float64), k_new=new[:, 0].transpose(0, 2, 1, 3), v_new=new[:, 1].transpose(0, 2, 1, 3))
                T._check_frame(ref, got, half, dict(case=case, slot=s, frame=f, forced=None if forced is None else forced[s].tolist()), worst, failures)
            lp = lp + 2
    finally:
        b.close()
    print("[ar fast path]", case, "worst err / bound", {q: round(v, 3) for q, v in worst.items()})
    assert not failures, failures
    assert n_near <= 0.01 * n_samp, (n_near, n_samp)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_twin_slots_of_one_launch_agree_bit_for_bit(engines, half):
    eng = engines(half)
    rng = np.random.default_rng(77 + int(half))
    b = T._make_batch(eng, 2, T.MODE_PER_STREAM)
    try:
        assert b.decode_path() == 1
        _start(b, [5000, 5000], rng, fill=np.tile(rng.integers(0, V, (1, T.DELAY)), (2, 1)))
        for f in range(2):
            code = np.full(2, int(rng.integers(0, V)))
            noise = np.tile((rng.exponential(size=(1, V + NCB * CBS)) + 1e-9).astype(np.float32), (2, 1))
            codes, _ = b.ar_decode_one(code, noise=noise)
            assert int(b.tap("ar_fail", (1,), np.int32)[0]) == 0
            fast = b.tap("fast_logits", (2, NCB, CBS))
            emb = b.tap("cached_audio_emb", (2, D))
            assert np.isfinite(fast).all()
            assert fast[0].tobytes() == fast[1].tobytes(), (f, float(np.abs(fast[0] - fast[1]).max()))
            np.testing.assert_array_equal(codes[0], codes[1])
            assert emb[0].tobytes() == emb[1].tobytes()
    finally:
        b.close()
