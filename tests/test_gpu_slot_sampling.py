"""Per-slot sampling: every slot of a batch owns its {temperature, top_p} pair in device memory (sva_stream_set_sampling), and every sampler
-- the four sampler kernels of kernels.hip and the two persistent decode kernels -- reads the pair of the row / stream it serves.

What is pinned:
  * the sampler kernels with per-row pairs, through the production launchers: tokens == kernel_refs.nucleus_token of each row under ITS pair
    (exact: test_slot_sampling_cpu.py asserts every row decidable under the pair it gets), row_slot indirection, null pointer == scalars;
  * a batch of mixed pairs == uniform batches, slot by slot and bit for bit, on the three decode paths;
  * a change under captured graphs takes effect at the next frame, top_p = 0 is greedy, the other slot is untouched;
  * stream_infer_many(sampling=...) == the same call on batches whose default is the utterance's pair; a restart puts the default back;
  * refusals change nothing;  generate() keeps its frame-0 quirk and otherwise follows slot 0's pair.

Equalities between runs are exact: both runs push the same rows through the same kernels at the same row positions, only the source of two
floats differs.  With SVA_SLOT_SAMPLING_TABLE=<path> the kernel test writes its parity table there."""
import functools
import os

import numpy as np
import pytest
import torch

import decode_tail_cases as G
import kernel_refs as R
from test_slot_sampling_cpu import mixed_cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N = 2048
PAIRS = ((0.7, 0.7), (1.0, 0.9), (1.3, 0.3))          # (temperature, top_p); the first is the batch default
F32 = np.float32


def _E():
    from streamvoiceanon_amd import engine as E
    return E


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


@functools.lru_cache(maxsize=None)
def _utt(seed, frames):
    from streamvoiceanon_amd.synth_audio import synth_utterance

    a = synth_utterance(seed, N * frames)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _prompt(seed, R_=107):
    from streamvoiceanon_amd.synth_audio import synth_prompt

    return synth_prompt(seed, R_)          # (ac, cc, style, timbre)


# =====================================================================================================================================
# 1. kernels, per-row pairs
# =====================================================================================================================================
SENT = -7
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    yield
    path = os.environ.get("SVA_SLOT_SAMPLING_TABLE")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("%-6s %-22s %-34s %-28s %5s %10s\n" % ("V", "launcher", "kernel chosen", "case", "rows", "mismatches"))
            for row in _TABLE:
                f.write("%-6d %-22s %-34s %-28s %5d %10d\n" % row)


def _kernel_chosen(small, V):
    """the kernel the launcher's dispatch picks for this V (kernels.hip: launch_sampler / launch_sampler_small)"""
    if small:
        return "sampler_bisect_kernel<256,4,2>"
    P = 1024
    while P < V:
        P <<= 1
    return "sampler_bisect_kernel<512,16,2>" if P == 8192 else "sampler_kernel (LDS sort, P=%d)" % P


def _launch_rows(small, L, Q, pairs, row_slot=None, temperature=0.7, top_p=0.7):
    """the production launcher over dense rows with sentinels around tok_raw / tok: -> tokens [rows]"""
    rows, V = L.shape
    pad, stride = 3, 2
    n = pad + rows * stride + pad
    tok_raw = np.full(n, SENT, np.int32)
    tok = np.full(n, SENT, np.int32) if small else None
    _E().test_sampler_rows(L.reshape(-1).copy(), rows, V, V, pairs=pairs, row_slot=row_slot, small=small, noise=Q.reshape(-1), ldn=V,
                           temperature=temperature, top_p=top_p, tok_raw=tok_raw, tok=tok, tok_stride=stride, tok_off=pad)
    written = np.zeros(n, bool)
    written[pad:pad + rows * stride:stride] = True
    assert (tok_raw[~written] == SENT).all(), "tok_raw written outside its rows"
    if small:
        assert (tok[~written] == SENT).all() and np.array_equal(tok, tok_raw)          # no forcing: tok = the sample
    return tok_raw[written]


def _want(L, Q, settings):
    return np.array([R.nucleus_token(L[r], Q[r], settings[r][1], settings[r][0])[0] for r in range(L.shape[0])], np.int32)


@pytest.mark.parametrize("small,V", [(True, V) for V in (1, 63, 1000, 1024)] + [(False, V) for V in (2048, 4097, 8191, 8192, 8193)])
def test_sampler_kernels_per_row_pairs(small, V):
    launcher = "launch_sampler_small" if small else "launch_sampler"
    for tag, L, Q, settings in mixed_cases(V):
        want = _want(L, Q, settings)
        pairs = [(temp, tp) for tp, temp in settings]
        got = _launch_rows(small, L, Q, pairs)
        _TABLE.append((V, launcher, _kernel_chosen(small, V), tag + " mixed pairs", L.shape[0], int((got != want).sum())))
        assert np.array_equal(got, want), (tag, V, np.nonzero(got != want)[0][:6])
        if tag == "random" and V in (1000, 8192):       # one pair for every row of the same launch: another answer, so the rows did read their own
            want_uni = _want(L, Q, [settings[0]] * L.shape[0])
            assert (want_uni != want).any()
            assert np.array_equal(_launch_rows(small, L, Q, [pairs[0]] * L.shape[0]), want_uni)


@pytest.mark.parametrize("small,V", [(True, 1000), (False, 8192), (False, 2048)])
def test_sampler_kernels_row_slot_indirection(small, V):
    """row r reads pair row_slot[r] of an array longer than the launch: shuffled slots, unused pairs in between"""
    tag, L, Q, settings = mixed_cases(V)[0]
    rows = L.shape[0]
    rng = np.random.default_rng(11)
    n_pairs = rows + 7
    row_slot = rng.permutation(n_pairs)[:rows].astype(np.int32)
    assert not np.array_equal(row_slot, np.arange(rows))
    pairs = [(55.0, 0.123)] * n_pairs                         # a pair no row is meant to read
    for r in range(rows):
        pairs[row_slot[r]] = (settings[r][1], settings[r][0])
    want = _want(L, Q, settings)
    got = _launch_rows(small, L, Q, pairs, row_slot=row_slot)
    _TABLE.append((V, "launch_sampler_small" if small else "launch_sampler", _kernel_chosen(small, V), tag + " shuffled row_slot", rows, int((got != want).sum())))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:6]


@pytest.mark.parametrize("small,V", [(True, 1000), (False, 8192)])
def test_sampler_kernels_null_pairs_use_the_scalars(small, V):
    L, Q = G.random_rows(V)
    L, Q = L[:G.RANDOM_ROWS], Q[:G.RANDOM_ROWS]
    tp, temp = G.RANDOM_SETTINGS[1]
    rows = L.shape[0]
    ref_raw = np.full(rows, SENT, np.int32)
    _E().test_sampler_launch(L.reshape(-1).copy(), rows, V, V, small=small, noise=Q.reshape(-1), ldn=V, temperature=temp, top_p=tp, tok_raw=ref_raw,
                             tok=np.full(rows, SENT, np.int32) if small else None)
    got = _launch_rows(small, L, Q, None, temperature=temp, top_p=tp)
    assert np.array_equal(got, ref_raw)
    assert np.array_equal(got, _want(L, Q, [(tp, temp)] * rows))
    _TABLE.append((V, "launch_sampler_small" if small else "launch_sampler", _kernel_chosen(small, V), "null pairs == scalars", rows, int((got != ref_raw).sum())))


def test_sampler_rows_hook_declines_bad_indices():
    """the hook's own bounds checks (host side, nothing is launched)"""
    L, Q = G.random_rows(63)
    with pytest.raises(RuntimeError):
        _launch_rows(True, L[:4], Q[:4], [(0.7, 0.7)] * 3)                                        # fewer pairs than rows
    with pytest.raises(RuntimeError):
        _launch_rows(True, L[:4], Q[:4], [(0.7, 0.7)] * 4, row_slot=np.array([0, 1, 4, 2], np.int32))      # slot outside the pairs
    with pytest.raises(RuntimeError):
        _launch_rows(True, L[:4], Q[:4], [(0.7, 0.7)] * 4, row_slot=np.array([0, -1, 1, 2], np.int32))


# =====================================================================================================================================
# batches
# =====================================================================================================================================
def _noise(n_steps, stride, seed=4242):
    rng = np.random.default_rng(seed)
    q = (rng.exponential(1.0, (n_steps, stride)) + 1e-9).astype(F32)
    q.setflags(write=False)
    return q


def _run(engine, B, n_steps, pairs=None, events=None, debug=None, noise=None, taps=(), utt_seed=7801, device_steps=False, **kw):
    """B slots with the same source and prompt; pairs[slot] = (temperature, top_p) or None, set before begin(); events[step] = calls made
    before that step: (slot, temperature, top_p) -> set_sampling; noise [n_steps, stride]: every slot gets the same row.  device_steps:
    sva_step_device on device buffers (the pipelined mode's stage graphs), synchronised after every step; the step's codes are then read
    from the slot's frame ring.  -> dict(pcm [steps, B, N], audio [steps, B, 8], codes [B][8, frames], path, taps...)"""
    E = _E()
    lib = E.load_library()
    if debug:
        lib.sva_debug_configure(debug.encode())          # (read at batch creation)
    try:
        b = E.Batch(engine, n_streams=B, **kw)
    finally:
        if debug:
            lib.sva_debug_configure(b"ar_batch=1,ar_persistent=1")
    rec = dict(path=b.decode_path(), pcm=[], audio=[], sampling=[])
    for t in taps:
        rec[t] = []
    try:
        ac, cc, st, tm = _prompt(2801)
        for s in range(B):
            b.prefill_prompt(s, cc, ac, st, tm, noise_seed=900)
        for s, p in enumerate(pairs or ()):
            if p is not None:
                b.set_sampling(s, *p)
        b.begin()
        src = _utt(utt_seed, n_steps)
        if device_steps:
            assert noise is None
            din = torch.from_numpy(np.repeat(src.reshape(n_steps, 1, N), B, axis=1).copy()).cuda()
            dout = torch.zeros(n_steps, B, N, device="cuda")
            torch.cuda.synchronize()
        for k in range(n_steps):
            for ev in (events or {}).get(k, ()):
                b.set_sampling(ev[0], temperature=ev[1], top_p=ev[2])
            if device_steps:
                b.step_device(din[k].data_ptr(), dout[k].data_ptr())
                b.sync()
                rec["pcm"].append(dout[k].cpu().numpy())
                rec["audio"].append(np.stack([b.pred_codes(s, 1)[:, 0] if b.frames_decoded(s) else np.zeros(8, np.int32) for s in range(B)]))
            else:
                x = np.repeat(src[None, k * N:(k + 1) * N], B, axis=0)
                nz = None if noise is None else np.repeat(noise[None, k:k + 1], B, axis=0)
                rec["pcm"].append(b.step(x, noise=nz))
                rec["audio"].append(b.tap("audio_codes", (B, 8, 1), np.int32)[:, :, 0].copy())
            for t in taps:
                rec[t].append(b.tap(t, (B, 8, 1000)).copy())
        b.sync()
        rec["codes"] = [b.pred_codes(s) for s in range(B)]
        rec["sampling"] = [b.sampling(s) for s in range(B)]
    finally:
        b.close()
    rec["pcm"], rec["audio"] = np.stack(rec["pcm"]), np.stack(rec["audio"])
    return rec


def _f32pair(p):
    return (float(F32(p[0])), float(F32(p[1])))


# ---- 2. mixed batch == uniform batches, on every decode path -------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,path,debug", [("b3_persistent_two_plus_one", 3, 1, None), ("b8_batched_persistent", 8, 2, None),
                                               ("b3_multi_launch", 3, 0, "ar_persistent=0")])
def test_mixed_batch_equals_uniform_batches(eng, name, B, path, debug):
    n_steps = 2 + 12
    noise = _noise(n_steps, 8192 + 8 * 1000)
    slot_pair = [PAIRS[s % 3] for s in range(B)]
    mixed = _run(eng, B, n_steps, pairs=[None if p == PAIRS[0] else p for p in slot_pair], debug=debug, noise=noise)
    assert mixed["path"] == path, "the case no longer runs the decode path it is named after"
    assert mixed["sampling"] == [_f32pair(p) for p in slot_pair]
    assert np.abs(mixed["pcm"][2:]).max() > 1e-3
    for p in PAIRS:
        uni = _run(eng, B, n_steps, debug=debug, noise=noise, temperature=p[0], top_p=p[1])         # never calls set_sampling
        assert uni["path"] == path and uni["sampling"] == [_f32pair(p)] * B
        for s in range(B):
            if slot_pair[s] != p:
                continue
            np.testing.assert_array_equal(mixed["codes"][s], uni["codes"][s], err_msg=f"codes of slot {s} under {p}")
            np.testing.assert_array_equal(mixed["audio"][:, s], uni["audio"][:, s])
            np.testing.assert_array_equal(mixed["pcm"][:, s], uni["pcm"][:, s], err_msg=f"pcm of slot {s} under {p}")
        assert uni["codes"][0].shape == (8, 12)
    # the pairs matter: same source, prompt and noise in every slot, so slots differ by their pair alone
    assert not np.array_equal(mixed["codes"][0], mixed["codes"][1]) and not np.array_equal(mixed["codes"][0], mixed["codes"][2])
    if B > 3:
        np.testing.assert_array_equal(mixed["codes"][0], mixed["codes"][3])


# ---- 3. greedy slot, and a change under captured graphs -----------------------------------------------------------------------------
GREEDY_SEED = 7801


def _greedy_script(eng, with_call, **kw):
    ev = {6: [(1, None, 0.0)]} if with_call else None
    return _run(eng, 2, 12, events=ev, taps=("fast_logits",), utt_seed=GREEDY_SEED, **kw)


def _assert_greedy(run, slot, first_step):
    worst = np.inf
    for k in range(first_step, run["pcm"].shape[0]):
        lg = run["fast_logits"][k][slot].astype(np.float64)          # [8, 1000], the rows the step's 8 codes were sampled from
        top2 = np.sort(lg, axis=1)[:, -2:]
        lead = (top2[:, 1] - top2[:, 0]) / np.maximum(np.abs(top2[:, 1]), 1e-30)
        worst = min(worst, float(lead.min()))
        assert (lead > 1e-4).all(), f"step {k}: a top logit leads by {lead.min():.3g} relative: pick another GREEDY_SEED"
        np.testing.assert_array_equal(run["audio"][k, slot], lg.argmax(axis=1), err_msg=f"step {k}: slot {slot} is not greedy")
    print(f"[slot sampling] greedy slot: smallest relative lead of a top logit {worst:.3g}")


@pytest.mark.parametrize("mode", ["use_graph", "pipeline"])
def test_greedy_slot_and_change_under_captured_graphs(eng, mode):
    kw = dict(use_graph=True) if mode == "use_graph" else dict(pipeline=True, device_steps=True)
    ctl = _greedy_script(eng, False, **kw)
    run = _greedy_script(eng, True, **kw)
    assert run["sampling"] == [_f32pair(PAIRS[0]), (_f32pair(PAIRS[0])[0], 0.0)]          # what was set (temperature None = the batch's)
    _assert_greedy(run, 1, 6)
    np.testing.assert_array_equal(run["audio"][:6], ctl["audio"][:6])                     # nothing changes before the call
    assert (run["audio"][6:, 1] != ctl["audio"][6:, 1]).any()                             # ... and slot 1 does after it
    np.testing.assert_array_equal(run["codes"][0], ctl["codes"][0])                       # slot 0 never notices
    np.testing.assert_array_equal(run["pcm"][:, 0], ctl["pcm"][:, 0])
    if mode == "use_graph":
        eager = _greedy_script(eng, True)
        for s in range(2):
            np.testing.assert_array_equal(run["codes"][s], eager["codes"][s])
            np.testing.assert_array_equal(run["pcm"][:, s], eager["pcm"][:, s])


# ---- 4. restart ----------------------------------------------------------------------------------------------------------------------
def test_stream_infer_many_per_utterance_sampling(wrap):
    chunks = (9, 14, 11, 8, 10)
    entries = [None, PAIRS[1], None, PAIRS[2], PAIRS[1]]
    sampling = [None if p is None else {"temperature": p[0], "top_p": p[1]} for p in entries]
    srcs = [_utt(7810 + u, c)[:N * (c - 1) + 300 + 100 * u] for u, c in enumerate(chunks)]
    prompts = [_prompt(2810 + u, (107, 70, 91, 64, 80)[u]) for u in range(5)]
    seeds = [40 + u for u in range(5)]
    seen = {}

    def on_step(k, feeds):
        for s, u, i in feeds:
            seen.setdefault(u, set()).add((s, k - i, wrap.batch.sampling(s)))

    many = wrap.stream_infer_many(srcs, prompts, n_slots=2, noise_seeds=seeds, slot_priming=False, sampling=sampling, on_step=on_step)
    where = {u: v for u, v in seen.items()}
    for u in range(5):        # one slot, one start step and one pair per utterance: its own entry, or the batch default after a bare restart
        assert len(where[u]) == 1
        assert next(iter(where[u]))[2] == _f32pair(entries[u] or PAIRS[0]), u
    assert next(iter(where[2]))[0] == next(iter(where[0]))[0] == 0 and next(iter(where[3]))[0] == 1      # utterances 2 / 3 follow 0 / 1 in their slots
    for p in PAIRS:
        seen.clear()
        uni = wrap.stream_infer_many(srcs, prompts, n_slots=2, noise_seeds=seeds, slot_priming=False, temperature=p[0], top_p=p[1], on_step=on_step)
        for u in range(5):
            assert {(s, k0) for s, k0, _ in seen[u]} == {(s, k0) for s, k0, _ in where[u]}        # the schedule depends on lengths only
            if (entries[u] or PAIRS[0]) == p:
                assert many[u].shape == (N * chunks[u],) and np.abs(many[u][2 * N:]).max() > 1e-3
                np.testing.assert_array_equal(many[u], uni[u], err_msg=f"utterance {u} under {p}")
    assert not np.array_equal(many[1][2 * N:], uni[1][2 * N:])          # (uni: the last pair, 1.3 / 0.3; utterance 1 ran under 1.0 / 0.9)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(eng):
    E = _E()
    lib = E.load_library()
    ctl = _run(eng, 2, 6, pairs=[None, PAIRS[1]])
    b = E.Batch(eng, n_streams=2)
    try:
        ac, cc, st, tm = _prompt(2801)
        for s in range(2):
            b.prefill_prompt(s, cc, ac, st, tm, noise_seed=900)
        b.set_sampling(1, *PAIRS[1])              # before sva_streams_begin
        b.begin()
        src = _utt(7801, 6)
        nan, inf = float("nan"), float("inf")
        for k in range(6):
            if k == 4:
                for args, word in (((-1, 1.0, 0.9), "slot"), ((2, 1.0, 0.9), "slot"), ((1, nan, 0.9), "temperature"), ((1, 1.0, nan), "top_p"),
                                   ((1, -0.5, 0.9), "temperature"), ((1, 1.0, -0.1), "top_p"), ((1, inf, 0.9), "temperature"), ((1, 1.0, inf), "top_p")):
                    with pytest.raises(RuntimeError) as ei:
                        b.set_sampling(*args)
                    msg = lib.sva_last_error().decode()
                    assert word in msg and msg in str(ei.value), (args, msg)
                    assert b.sampling(1) == _f32pair(PAIRS[1]) and b.sampling(0) == _f32pair(PAIRS[0])
                for slot in (-1, 2):
                    with pytest.raises(RuntimeError):
                        b.sampling(slot)
                    assert "slot" in lib.sva_last_error().decode()
            out = b.step(np.repeat(src[None, k * N:(k + 1) * N], 2, axis=0))
            np.testing.assert_array_equal(b.tap("audio_codes", (2, 8, 1), np.int32)[:, :, 0], ctl["audio"][k])
            np.testing.assert_array_equal(out, ctl["pcm"][k])
        b.sync()
    finally:
        b.close()


# ---- 6. generate ---------------------------------------------------------------------------------------------------------------------
def test_generate_follows_slot_pair_after_frame0(eng):
    from streamvoiceanon_amd.synth_audio import frame_noise

    E = _E()
    useed, S = 881, 10
    ac, cc, style, timbre = _prompt(2301, 24)
    src_codes = (np.arange(S, dtype=np.int64) * 2654435761 % 8192).astype(np.int64)
    noise = np.stack([np.concatenate([frame_noise(useed, s)[0], frame_noise(useed, s)[1].reshape(-1)]) for s in range(S)])

    def gen(batch_kw, pair=None):
        b = E.Batch(eng, n_streams=1, delay=2, **batch_kw)
        try:
            if pair is not None:
                b.set_sampling(0, *pair)
            codes = b.generate(cc, ac, src_codes, style, timbre, noise=noise)
            return codes, b.sampling(0)
        finally:
            b.close()

    want, _ = gen(dict(temperature=1.0, top_p=0.9))
    got, after = gen({}, pair=(1.0, 0.9))
    dflt, _ = gen({})
    np.testing.assert_array_equal(got, want)
    assert after == _f32pair((1.0, 0.9))                             # the slot's own pair is back after the prefill's decode
    np.testing.assert_array_equal(got[:, 0], dflt[:, 0])             # frame 0: 0.7 / 0.7 whatever the slot holds
    assert (got[:, 1:] != dflt[:, 1:]).any()
