"""Offline conversion of many utterances in one batch: the runs arm of ar_prefill_attention_kernel against fp64 (through
E.test_prefill_attention_runs), sva_generate_many / Batch.generate_many against the CPU oracle on every decode path with ragged prompt and
source lengths, and InferenceWrapper.infer_many against infer of each utterance alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PCM_TOL = 5e-5
DELAY = 2
# (prompt seed, R, utterance seed, S): ragged on both sides; S = 3 is the shortest legal source (delay + 1)
UTTS = [(2301, 24, 881, 10), (2312, 39, 892, 3), (2313, 31, 893, 14), (2314, 24, 894, 5), (2315, 48, 895, 12)]


@pytest.fixture(scope="module")
def wrap(weights0):
    from streamvoiceanon_amd.infer_arvc import InferenceWrapper

    w = InferenceWrapper(weights=weights0)
    yield w
    w.close()
    w.engine.close()


@pytest.fixture(scope="module")
def eng(wrap):
    return wrap.engine


@pytest.fixture(scope="module")
def eng_fp16(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0, ar_dtype=1)
    yield e
    e.close()


def _src_codes(S):
    return (np.arange(S, dtype=np.int64) * 2654435761 % 8192).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _prompt(seed, R):
    from streamvoiceanon_amd.synth_audio import synth_prompt

    ac, cc, style, timbre = synth_prompt(seed, R)
    for a in (ac, cc, style, timbre):
        a.setflags(write=False)
    return cc, ac, style, timbre              # generate_many's order


@functools.lru_cache(maxsize=None)
def _noise_row(useed, s):
    from streamvoiceanon_amd.synth_audio import frame_noise

    ns, nf = frame_noise(useed, s)
    return np.concatenate([ns, nf.reshape(-1)]).astype(np.float32)


def _noise_block(useeds, s_max):
    """host noise of generate_many: [S_max][n][vocab + 8 * codebook_size], frame-major; slot i reads frame_noise(useed_i, frame)"""
    return np.stack([np.stack([_noise_row(u, s) for u in useeds]) for s in range(s_max)])


_ORACLE = {}


def _oracle(weights0, pseed, R, useed, S, temperature=0.7, top_p=0.7, src=None):
    """DualAR.generate of one utterance under its own noise (computed once per case, shared between the tests)"""
    from oracle import sva_oracle as O
    from streamvoiceanon_amd.synth_audio import frame_noise

    key = (pseed, R, useed, S, temperature, top_p, None if src is None else tuple(int(x) for x in src))
    if key not in _ORACLE:
        cc, ac, style, timbre = _prompt(pseed, R)
        sc = _src_codes(S) if src is None else np.asarray(src, dtype=np.int64)
        ar = O.DualAR(weights0, temperature=temperature, top_p=top_p)
        ref = ar.generate(torch.from_numpy(cc.copy()), torch.from_numpy(ac.copy()), torch.from_numpy(sc), torch.from_numpy(style.copy()),
                          torch.from_numpy(timbre.copy()), DELAY, noise_fn=lambda s_: tuple(torch.from_numpy(a) for a in frame_noise(useed, s_)))
        out = ref.numpy().astype(np.int32).reshape(8, S)
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _generate_many_raw(b, prompts, sources, seeds, noise, n=None):
    """sva_generate_many through ctypes with a 16-int sentinel behind every codes_out[i] -> (codes list, sentinels intact)"""
    from streamvoiceanon_amd import engine as E

    lib = E.load_library()
    k = len(sources)
    ccs = [np.ascontiguousarray(p[0], dtype=np.int64) for p in prompts]
    acs = [np.ascontiguousarray(p[1], dtype=np.int32) for p in prompts]
    srcs = [np.ascontiguousarray(s, dtype=np.int64) for s in sources]
    st = np.ascontiguousarray(np.stack([p[2] for p in prompts]), dtype=np.float32)
    tm = np.ascontiguousarray(np.stack([p[3] for p in prompts]), dtype=np.float32)
    R = np.array([c.shape[0] for c in ccs], dtype=np.int32)
    S = np.array([s.shape[0] for s in srcs], dtype=np.int32)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    outs = [np.full(8 * int(s) + 16, -77, dtype=np.int32) for s in S]
    arr = lambda xs: (ctypes.c_void_p * k)(*[x.ctypes.data for x in xs])
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.sva_generate_many(b.h, k if n is None else n, arr(ccs), arr(acs), vp(R), arr(srcs), vp(S), vp(st), vp(tm), vp(sd), vp(nz), arr(outs))
    if rc != 0:
        raise RuntimeError(lib.sva_last_error().decode("utf-8", "replace"))
    intact = all((o[8 * int(s):] == -77).all() for o, s in zip(outs, S))
    return [o[:8 * int(s)].reshape(8, int(s)).copy() for o, s in zip(outs, S)], intact


def _batch(engine, B, debug=None, **kw):
    from streamvoiceanon_amd import engine as E

    lib = E.load_library()
    if debug:
        lib.sva_debug_configure(debug.encode())          # (read at batch creation)
    try:
        return E.Batch(engine, n_streams=B, delay=DELAY, **kw)
    finally:
        if debug:
            lib.sva_debug_configure(b"ar_batch=1,ar_persistent=1")


def _case(idx):
    utts = [UTTS[i] for i in idx]
    prompts = [_prompt(p, R) for p, R, _, _ in utts]
    sources = [_src_codes(S) for _, _, _, S in utts]
    useeds = [u for _, _, u, _ in utts]
    return utts, prompts, sources, useeds, _noise_block(useeds, max(S for _, _, _, S in utts))


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
RUNS = [(2, 0, 273, 0),         # more than 256 keys: a wave reaches its second key block
        (0, 0, 7, 273),         # shorter than one tile
        (1, 37, 65, 280),       # non-zero pos0, tile tail of 1 row
        (0, 7, 16, 350)]        # exactly one tile, continuing slot 0; rows 345 .. 349 belong to nobody
SENTINEL = np.float32(777.25)


@pytest.mark.parametrize("half_kv", [False, True])
def test_prefill_attention_runs_vs_fp64(half_kv, record_property):
    """the RUNS arm of ar_prefill_attention_kernel: a packed pass over rows of three slots, out of slot order and with a gap, against fp64
    softmax(QK^T / 8) V per run with the causal mask of its positions, and against the single-run arm called once per run"""
    from streamvoiceanon_amd import engine as E

    H, S, n_slots, total = 12, 640, 3, 366
    rng = np.random.default_rng(640 + int(half_kv))
    q = rng.standard_normal((total, H * 64)).astype(np.float32) * 1.5
    cache = rng.standard_normal((n_slots, 2, H, S, 64)).astype(np.float32)
    out = np.full((total, H * 64), SENTINEL, dtype=np.float32)
    single = np.full((total, H * 64), SENTINEL, dtype=np.float32)
    assert E.test_prefill_attention_runs(RUNS, total, H, S, n_slots, half_kv, q, cache, out, single) is False
    cc = cache.astype(np.float16) if half_kv else cache
    covered = np.zeros(total, dtype=bool)
    worst = worst_single = 0.0
    for slot, pos0, M, row0 in RUNS:
        L = pos0 + M
        q3 = q[row0:row0 + M].astype(np.float64).reshape(M, H, 64).transpose(1, 0, 2)
        k3 = cc[slot, 0, :, :L].astype(np.float64)
        v3 = cc[slot, 1, :, :L].astype(np.float64)
        s = q3 @ k3.transpose(0, 2, 1) / 8.0
        mask = np.arange(L)[None, :] > (pos0 + np.arange(M))[:, None]
        s[:, mask] = -np.inf
        p = np.exp(s - s.max(-1, keepdims=True))
        want = ((p / p.sum(-1, keepdims=True)) @ v3).transpose(1, 0, 2).reshape(M, H * 64)
        worst = max(worst, float(np.abs(out[row0:row0 + M] - want).max()))
        worst_single = max(worst_single, float(np.abs(single[row0:row0 + M] - want).max()))
        covered[row0:row0 + M] = True
    identical = bool(np.array_equal(out, single))
    print("prefill attention runs", dict(half_kv=half_kv, max_err=worst, max_err_single=worst_single, bit_identical_to_single_run=identical))
    record_property("prefill_runs", dict(half_kv=half_kv, max_err=worst, bit_identical_to_single_run=identical))
    assert worst < 2e-5
    assert worst_single < 2e-5 and float(np.abs(out[covered] - single[covered]).max()) < 2e-5
    assert (~covered).sum() == 5 and (out[~covered] == SENTINEL).all() and (single[~covered] == SENTINEL).all()


def test_prefill_attention_runs_refusals():
    from streamvoiceanon_amd import engine as E

    H, S, n_slots, total = 2, 64, 2, 40
    rng = np.random.default_rng(3)
    q = rng.standard_normal((total, H * 64)).astype(np.float32)
    cache = rng.standard_normal((n_slots, 2, H, S, 64)).astype(np.float32)
    for runs in ([(0, 0, 16, 0), (1, 0, 16, 8)],          # overlapping row ranges
                 [(0, 50, 16, 0)]):                       # pos0 + M > S
        out = np.full((total, H * 64), SENTINEL, dtype=np.float32)
        q0, c0 = q.copy(), cache.copy()
        assert E.test_prefill_attention_runs(runs, total, H, S, n_slots, False, q, cache, out) is True
        assert (out == SENTINEL).all() and np.array_equal(q, q0) and np.array_equal(cache, c0)


# ---- 2. generate_many against the oracle on every decode path ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(UTTS)))
def test_single_stream_generate_equals_oracle(eng, weights0, i):
    """the inputs of the batch cases, through the existing one-stream Batch.generate: each equals the oracle alone"""
    pseed, R, useed, S = UTTS[i]
    cc, ac, style, timbre = _prompt(pseed, R)
    b = _batch(eng, 1)
    try:
        codes = b.generate(cc, ac, _src_codes(S), style, timbre, noise=_noise_block([useed], S)[:, 0])
    finally:
        b.close()
    np.testing.assert_array_equal(codes, _oracle(weights0, pseed, R, useed, S))


@pytest.mark.parametrize("idx,debug,path", [((0, 1, 2), None, 1), ((0, 1, 2, 3, 4), "ar_batch=2", 2), ((0, 1, 2, 3, 4), "ar_persistent=0,ar_batch=0", 0)],
                         ids=["B3-persistent", "B5-batched-persistent", "B5-multi-launch"])
def test_generate_many_equals_oracle(eng, weights0, idx, debug, path):
    utts, prompts, sources, useeds, noise = _case(idx)
    b = _batch(eng, len(idx), debug)
    try:
        assert b.decode_path() == path and b.uses_persistent_decode() == (path != 0)
        codes, intact = _generate_many_raw(b, prompts, sources, useeds, noise)
        again = b.generate_many(prompts, sources, noise_seeds=useeds, noise=noise)          # the Python entry, on the state the first call left
    finally:
        b.close()
    assert intact, "sva_generate_many wrote behind a codes_out"
    for k, (pseed, R, useed, S) in enumerate(utts):
        assert codes[k].shape == (8, S) and again[k].shape == (8, S) and again[k].dtype == np.int32
        np.testing.assert_array_equal(codes[k], _oracle(weights0, pseed, R, useed, S), err_msg="slot %d" % k)
        np.testing.assert_array_equal(again[k], codes[k], err_msg="slot %d, second call" % k)


def test_generate_many_fp16(eng, eng_fp16, record_property):
    idx = (0, 1, 2, 3, 4)
    utts, prompts, sources, useeds, noise = _case(idx)
    got = {}
    for name, e in (("fp32", eng), ("fp16", eng_fp16)):
        b = _batch(e, len(idx))
        try:
            got[name] = b.generate_many(prompts, sources, noise_seeds=useeds, noise=noise)
        finally:
            b.close()
    same0 = [bool(np.array_equal(a[:, 0], c[:, 0])) for a, c in zip(got["fp16"], got["fp32"])]
    for k, (_, _, _, S) in enumerate(utts):
        assert got["fp16"][k].shape == (8, S) and got["fp16"][k].dtype == np.int32
        assert (got["fp16"][k] >= 0).all() and (got["fp16"][k] < 1000).all()
    record_property("generate_many_fp16", dict(frame0_equal_to_fp32=same0))
    print("generate_many fp16: frame 0 equal to the fp32 run per slot:", same0)


# ---- 3. a finished slot is independent of its neighbours --------------------------------------------------------------------------------
def test_finished_slot_is_independent_of_neighbours(eng):
    utts, prompts, sources, useeds, _ = _case((0, 1, 2))
    b = _batch(eng, 3)
    try:
        a = b.generate_many(prompts, sources, noise_seeds=useeds)
        rng = np.random.default_rng(11)
        other = [rng.integers(0, 8192, 4).astype(np.int64), sources[1], rng.integers(0, 8192, 25).astype(np.int64)]
        c = b.generate_many(prompts, other, noise_seeds=useeds)
    finally:
        b.close()
    assert a[1].shape == (8, 3) and c[0].shape == (8, 4) and c[2].shape == (8, 25)
    np.testing.assert_array_equal(a[1], c[1])


# ---- 4. frame-0 rule and per-slot sampling ----------------------------------------------------------------------------------------------
def test_frame0_rule_and_per_slot_sampling(eng, weights0):
    utts, prompts, sources, useeds, noise = _case((0, 2, 4))
    b = _batch(eng, 3)
    try:
        b.set_sampling(1, 1.3, 0.95)
        codes = b.generate_many(prompts, sources, noise_seeds=useeds, noise=noise)
        pair = b.sampling(1)
    finally:
        b.close()
    for k, (pseed, R, useed, S) in enumerate(utts):
        kw = dict(temperature=1.3, top_p=0.95) if k == 1 else {}
        np.testing.assert_array_equal(codes[k], _oracle(weights0, pseed, R, useed, S, **kw), err_msg="slot %d" % k)
    pseed, R, useed, S = utts[1]
    dflt = _oracle(weights0, pseed, R, useed, S)
    np.testing.assert_array_equal(codes[1][:, 0], dflt[:, 0])            # frame 0 at 0.7 / 0.7 whatever the slot's pair
    assert (codes[1] != dflt).any()
    assert pair == pytest.approx((1.3, 0.95), rel=1e-6)


# ---- 5. the reference's own fixture in slot 0 -------------------------------------------------------------------------------------------
def test_generate_many_reference_fixture_in_slot0(eng):
    g = load_golden("offline_s0")
    assert int(g["delay"]) == DELAY
    useed = int(g["audio_seed"])
    S = g["src_codes"].shape[0]
    assert S == 12
    _, prompts, sources, useeds, _ = _case((0, 2))
    prompts = [_prompt(int(g["prompt_seed"]), int(g["prompt_frames"]))] + prompts
    sources = [np.asarray(g["src_codes"], dtype=np.int64)] + sources
    useeds = [useed] + useeds
    s_max = max(s.shape[0] for s in sources)
    b = _batch(eng, 3, voc_max_frames=s_max)
    try:
        codes = b.generate_many(prompts, sources, noise_seeds=useeds, noise=_noise_block(useeds, s_max))
        np.testing.assert_array_equal(codes[0], g["codes"].reshape(8, S))
        padded = np.zeros((3, 8, s_max), np.int32)
        for k, c in enumerate(codes):
            padded[k, :, :c.shape[1]] = c
        pcm = b.vocode_window(padded)
    finally:
        b.close()
    np.testing.assert_allclose(pcm[0, 2048 * 11:2048 * 12], g["pcm_last"], atol=PCM_TOL)


# ---- 6. refusals change nothing -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(eng, weights0):
    utts, prompts, sources, useeds, noise = _case((0, 1, 2))
    b = _batch(eng, 3)
    try:
        first, _ = _generate_many_raw(b, prompts, sources, useeds, noise)
        with pytest.raises(RuntimeError, match="n == n_streams"):
            _generate_many_raw(b, prompts[:2], sources[:2], useeds[:2], noise[:, :2])
        with pytest.raises(RuntimeError, match="source length must exceed the delay"):
            _generate_many_raw(b, prompts, [sources[0], _src_codes(DELAY), sources[2]], useeds, noise)
        long_prompt = _prompt(2399, 1000)                # M = 33 + 2 * 1002 + 1 = 2038 rows fit a pass; + 2 * (10 - 1) positions do not fit the cache
        with pytest.raises(RuntimeError, match="exceed the 2048-position KV cache"):
            _generate_many_raw(b, [long_prompt, prompts[1], prompts[2]], sources, useeds, noise)
        after, intact = _generate_many_raw(b, prompts, sources, useeds, noise)
    finally:
        b.close()
    assert intact
    for k, (pseed, R, useed, S) in enumerate(utts):
        np.testing.assert_array_equal(first[k], _oracle(weights0, pseed, R, useed, S))
        np.testing.assert_array_equal(after[k], first[k])


# ---- 7. a source as long as the prediction history ----------------------------------------------------------------------------------------
def _batch_with_hist_cap(engine, B, cap):
    """a batch whose history rings hold `cap` frames (SVA_DEBUG hist_cap, read at batch creation; the default is back before anything runs);
    with buffer_frames = 16 the batch's own rule buffer_frames + delay + chunk < hist_cap admits no ring below 32"""
    from streamvoiceanon_amd import engine as E

    lib = E.load_library()
    assert lib.sva_debug_configure(("hist_cap=%d" % cap).encode()) == 0
    try:
        return E.Batch(engine, n_streams=B, delay=DELAY, buffer_frames=16)
    finally:
        lib.sva_debug_configure(b"hist_cap=4096")


def test_source_as_long_as_the_history(eng):
    """S == hist_cap is legal for both entries (a slot parks in column S_i only while a longer one runs, and S_max <= hist_cap): a 32-frame source
    on 32-column rings, alone and next to a 5-frame slot that parks beside the full ring, gives the codes of the default rings; 33 frames are
    refused by both entries and change nothing"""
    CAP = 32
    prompts = [_prompt(2301, 24), _prompt(2314, 24)]
    useeds = [881, 894]
    sources = [_src_codes(CAP), _src_codes(5)]
    too_long = _src_codes(CAP + 1)
    noise = _noise_block(useeds, CAP + 1)
    cc, ac, style, timbre = prompts[0]
    got = {}
    for cap in (4096, CAP):
        b = _batch_with_hist_cap(eng, 1, cap)
        try:
            one = b.generate(cc, ac, sources[0], style, timbre, noise=noise[:CAP, 0])
            if cap == CAP:
                with pytest.raises(RuntimeError, match="prediction history"):
                    b.generate(cc, ac, too_long, style, timbre, noise=noise[:, 0])
                np.testing.assert_array_equal(b.generate(cc, ac, sources[0], style, timbre, noise=noise[:CAP, 0]), one)
        finally:
            b.close()
        b = _batch_with_hist_cap(eng, 2, cap)
        try:
            many = b.generate_many(prompts, sources, noise_seeds=useeds, noise=noise[:CAP])
            if cap == CAP:
                with pytest.raises(RuntimeError, match="prediction history"):
                    b.generate_many(prompts, [too_long, sources[1]], noise_seeds=useeds, noise=noise)
                again = b.generate_many(prompts, sources, noise_seeds=useeds, noise=noise[:CAP])
                for k in range(2):
                    np.testing.assert_array_equal(again[k], many[k], err_msg="slot %d after the refusal" % k)
        finally:
            b.close()
        got[cap] = (one, many)
    assert got[CAP][0].shape == (8, CAP) and got[CAP][1][0].shape == (8, CAP) and got[CAP][1][1].shape == (8, 5)
    np.testing.assert_array_equal(got[CAP][0], got[4096][0])
    for k in range(2):
        np.testing.assert_array_equal(got[CAP][1][k], got[4096][1][k], err_msg="slot %d" % k)


# ---- 8. infer_many end to end -------------------------------------------------------------------------------------------------------------
def test_infer_many_equals_infer_alone(wrap, record_property):
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.stream_pool import plan_offline_waves
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

    frames = [3, 5, 9, 12, 12]
    seeds = [7101 + i for i in range(len(frames))]
    sources = [synth_utterance(s, 2048 * f) for s, f in zip(seeds, frames)]
    prompts = [synth_prompt(2401 + i, 24 + 5 * i) for i in range(len(frames))]            # (ac, cc, style, timbre) as calculate_prompt returns them
    wavs = wrap.infer_many(sources, prompts=prompts, n_slots=3, delay=DELAY, noise_seeds=seeds)
    assert len(wavs) == len(frames)
    alone = [np.asarray(wrap.infer(s, prompt=p, delay=DELAY, save_result=False, noise_seed=sd), np.float32).reshape(-1)
             for s, p, sd in zip(sources, prompts, seeds)]
    single_codes = [wrap.encode_content(s) for s in sources]
    flips = []
    for wave in plan_offline_waves(frames, 3):
        s_max = max(frames[i] for i in wave)
        Wp = ((s_max + 3) // 4) * 4
        b = E.Batch(wrap.engine, n_streams=len(wave), encode_window_frames=Wp, voc_max_frames=s_max, delay=DELAY)
        try:
            buf = np.zeros((len(wave), Wp * 2048), np.float32)
            for k, i in enumerate(wave):
                buf[k, :frames[i] * 2048] = sources[i]
            batched = b.encode_window(buf)
            flipped = [i for k, i in enumerate(wave) if not np.array_equal(batched[k, :frames[i]], single_codes[i])]
            if flipped:
                # a content code on a BSQ margin below 1e-5: the rest of the path is compared from the single encode's codes
                flips += flipped
                pr = [(p[1].reshape(-1), p[0].reshape(8, -1), p[2].reshape(-1), p[3].reshape(32, -1)) for p in (prompts[i] for i in wave)]
                codes = b.generate_many(pr, [single_codes[i] for i in wave], noise_seeds=[seeds[i] for i in wave])
                padded = np.zeros((len(wave), 8, s_max), np.int32)
                for k, c in enumerate(codes):
                    padded[k, :, :c.shape[1]] = c
                pcm = b.vocode_window(padded)
                for k, i in enumerate(wave):
                    wavs[i] = pcm[k, :frames[i] * 2048].copy()
        finally:
            b.close()
    record_property("infer_many_content_flips", flips)
    print("infer_many: utterances with a flipped content code between batched and single encode:", flips)
    for i, f in enumerate(frames):
        assert wavs[i].shape == (2048 * f,) and alone[i].shape == (2048 * f,), i
        np.testing.assert_allclose(wavs[i], alone[i], atol=PCM_TOL, err_msg="utterance %d" % i)
