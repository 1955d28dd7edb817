"""sva_stream_restart / sva_stream_retire / sva_stream_state: a single slot of a running batch gets a new utterance, or idles, while
the other slots keep running.

What is pinned:
  * a restarted slot IS a fresh slot -- against the reference's golden stream across its re-prefill (explicit host noise), and against
    a twin slot of the same batch that carries the same utterance from the batch's start (device RNG), on every decode path;
  * every other slot is bit-identical to a control run of the same batch without the call;
  * a retired slot outputs exact zeros, reads nothing (NaN input), raises nothing, and comes back through a restart;
  * refusals change nothing;
  * InferenceWrapper.stream_infer_many (continuous batching over ragged utterances) = stream_infer of each utterance alone.

Tolerances: codes, positions and frame counts are compared exactly; PCM of the restarted slot against its twin / the reference within the
project's fp32 vocoder tolerance PCM_TOL (tests/test_gpu_parity.py: 5e-5 on the tanh output) -- the slot's vocoder state is primed in a
whole-batch run of its own, so bit-equality with the twin is reported (record_property "pcm_bit_equal"), not asserted."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PCM_TOL = 5e-5
N = 2048
K0 = 5


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


@functools.lru_cache(maxsize=None)
def _utt(seed, frames):
    from streamvoiceanon_amd.synth_audio import synth_utterance

    a = synth_utterance(seed, N * frames)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _prompt(seed, R=107):
    from streamvoiceanon_amd.synth_audio import synth_prompt

    return synth_prompt(seed, R)          # (ac, cc, style, timbre)


def _run(engine, B, n_steps, feeds, prompts, seeds, events=None, chunk=1, noise=None, edits=False, device_steps=False, **kw):
    """One batch over n_steps.  feeds[slot] = [(first step, audio | None)]: the slot reads the segment that began last, from its start;
    None = NaN chunks, past a segment's end = zeros.  events[step] = calls made BEFORE that step: ("restart", slot, prompt, seed) or
    ("retire", slot).  noise(step) -> host noise [B, chunk, stride] or None (device RNG).  device_steps: sva_step_device on device
    buffers without taps (the pipelined mode keeps overlapping)."""
    from streamvoiceanon_amd import engine as E

    n = N * chunk
    b = E.Batch(engine, n_streams=B, chunk_frames=chunk, **kw)
    for s in range(B):
        ac, cc, st, tm = prompts[s]
        b.prefill_prompt(s, cc, ac, st, tm, noise_seed=seeds[s])
    if edits:
        b.set_sampler_edits(previous_tokens=np.arange(9 * 6, dtype=np.int32).reshape(9, 6) * 7 % 1000, repetition_penalty=1.3, suppress_tokens=[3, 11])
    b.begin()
    X = np.zeros((n_steps, B, n), np.float32)
    for k in range(n_steps):
        for s in range(B):
            k0, a = [seg for seg in feeds[s] if seg[0] <= k][-1]
            if a is None:
                X[k, s] = np.nan
            elif (k - k0 + 1) * n <= a.shape[0]:
                X[k, s] = a[(k - k0) * n:(k - k0 + 1) * n]
    rec = dict(pcm=[], content=[], audio=[], state=[], path=b.decode_path())
    if device_steps:
        din, dout = torch.from_numpy(X).cuda(), torch.zeros(n_steps, B, n, device="cuda")
        torch.cuda.synchronize()
    for k in range(n_steps):
        for ev in (events or {}).get(k, ()):
            if ev[0] == "restart":
                ac, cc, st, tm = ev[2]
                b.restart(ev[1], cc, ac, st, tm, noise_seed=ev[3])
            else:
                b.retire(ev[1])
        if device_steps:
            b.step_device(din[k].data_ptr(), dout[k].data_ptr())
        else:
            rec["pcm"].append(b.step(X[k], noise=None if noise is None else noise(k)))
            rec["content"].append(b.tap("content_codes", (B, chunk), np.int32).copy())
            rec["audio"].append(b.tap("audio_codes", (B, 8, chunk), np.int32).copy())
        rec["state"].append([b.stream_state(s) for s in range(B)])
    b.sync()                                            # raises on any deferred error (persistent-kernel timeout, range flag)
    if device_steps:
        rec["pcm"] = list(dout.cpu().numpy())
    rec["codes"] = [b.pred_codes(s) for s in range(B)]
    rec["last_pos"] = b.tap("last_pos", (B,), np.int32).copy()
    b.close()
    rec["pcm"] = np.stack(rec["pcm"])
    rec["state"] = np.array(rec["state"])               # [step][slot][phase, frames]
    if not device_steps:
        rec["content"], rec["audio"] = np.stack(rec["content"]), np.stack(rec["audio"])
    return rec


def _assert_untouched(run, ctl, slots, what="control"):
    for s in slots:
        np.testing.assert_array_equal(run["pcm"][:, s], ctl["pcm"][:, s], err_msg=f"pcm of slot {s} vs {what}")
        np.testing.assert_array_equal(run["codes"][s], ctl["codes"][s], err_msg=f"codes of slot {s} vs {what}")
        np.testing.assert_array_equal(run["state"][:, s], ctl["state"][:, s])
        if isinstance(run["content"], np.ndarray):
            np.testing.assert_array_equal(run["content"][:, s], ctl["content"][:, s])
            np.testing.assert_array_equal(run["audio"][:, s], ctl["audio"][:, s])


def _assert_twin(run, slot, k0, twin=0, chunk=1, delay=2, n_cmp=None, record_property=None, tag=""):
    """slot restarted before step k0 with the twin's utterance / prompt / seed: step k0 + i of the slot = step i of the twin"""
    n_steps = run["pcm"].shape[0]
    n_cmp = n_steps - k0 if n_cmp is None else n_cmp
    assert n_cmp >= 6
    zero_steps = -(-delay // chunk)
    np.testing.assert_array_equal(run["state"][k0:k0 + n_cmp, slot], run["state"][:n_cmp, twin])          # phase and frames
    assert tuple(run["state"][k0 + zero_steps - 1, slot]) == (2, 0)                                        # activated at the end of that step
    assert (run["state"][k0:k0 + zero_steps - 1, slot, 0] == 1).all()
    assert run["state"][k0 + n_cmp - 1, slot, 1] == (n_cmp - zero_steps) * chunk > 0
    assert not run["pcm"][k0:k0 + zero_steps, slot].any()                                                  # exact zeros while the delay fills
    assert np.abs(run["pcm"][k0 + zero_steps:k0 + n_cmp, slot]).max() > 1e-3
    if isinstance(run["content"], np.ndarray):
        np.testing.assert_array_equal(run["content"][k0:k0 + n_cmp, slot], run["content"][:n_cmp, twin])
        np.testing.assert_array_equal(run["audio"][k0 + zero_steps:k0 + n_cmp, slot], run["audio"][zero_steps:n_cmp, twin])
    nf = (n_cmp - zero_steps) * chunk
    assert k0 + n_cmp == n_steps and run["codes"][slot].shape == (8, nf)                                   # its frame ring restarted with the stream
    np.testing.assert_array_equal(run["codes"][slot], run["codes"][twin][:, :nf])
    a, t = run["pcm"][k0:k0 + n_cmp, slot], run["pcm"][:n_cmp, twin]
    np.testing.assert_allclose(a, t, rtol=0, atol=PCM_TOL)
    if record_property is not None:
        record_property("pcm_bit_equal" + tag, bool(np.array_equal(a, t)))
        record_property("pcm_max_abs_diff" + tag, float(np.abs(a - t).max()))
    print(f"[stream restart] slot {slot}{tag}: pcm bit-equal to its twin: {np.array_equal(a, t)}, max |d| = {np.abs(a - t).max():.3g}")


# ---- 1. restarted slot = fresh slot, against the reference ---------------------------------------------------------------------
def test_restarted_slot_equals_fresh_slot_vs_reference_golden(eng):
    from streamvoiceanon_amd.synth_audio import frame_noise

    g0, g1 = load_golden("stream_s0"), load_golden("stream_reprefill")
    assert int(g1["max_seq_frames"]) == 136 and int(g1["delay"]) == 2 and int(g1["chunk"]) == 1 and int(g1["n_chunks"]) == 30
    u0, u1 = int(g0["audio_seed"]), int(g1["audio_seed"])
    utt0, utt1 = _utt(u0, int(g0["n_chunks"])), _utt(u1, int(g1["n_chunks"]))
    p0, p1 = _prompt(int(g0["prompt_seed"]), int(g0["prompt_frames"])), _prompt(int(g1["prompt_seed"]), int(g1["prompt_frames"]))
    k_re, n_steps = 7, 37
    kw = dict(max_seq_frames=136, buffer_frames=int(g1["buffer_frames"]), delay=2)
    feeds = [[(0, utt0)], [(0, utt1), (k_re, utt1)]]
    events = {k_re: [("restart", 1, p1, u1)]}

    def noise(k):       # per slot: the noise of the frame it decodes in step k (its own stream's frame counter)
        rows = []
        for seed, frame in ((u0, max(k - 2, 0)), (u1, max(k - 2, 0) if k < k_re else max(k - k_re - 2, 0))):
            ns, nf = frame_noise(seed, frame)
            rows.append(np.concatenate([ns, nf.reshape(-1)])[None])
        return np.stack(rows)

    r = _run(eng, 2, n_steps, feeds, [p0, p1], [u0, u1], events=events, noise=noise, **kw)
    np.testing.assert_array_equal(r["content"][k_re:, 1, 0], g1["content_codes"])
    np.testing.assert_array_equal(r["audio"][k_re + 2:, 1, :, 0].T, g1["audio_codes"])           # all 28 frames, across the fixture's re-prefill
    assert int(r["last_pos"][1]) == int(g1["final_pos"])
    for k, idx in enumerate(g1["pcm_full_idx"]):
        np.testing.assert_allclose(r["pcm"][k_re + int(idx), 1], g1["pcm_full"][k], rtol=0, atol=PCM_TOL)
    assert not r["pcm"][k_re:k_re + 2, 1].any()
    np.testing.assert_array_equal(r["state"][-1, 1], [2, 28])
    # slot 0 against a control run without the restart (slot 1 simply continues), device RNG
    a = _run(eng, 2, n_steps, feeds, [p0, p1], [u0, u1], events=events, **kw)
    c = _run(eng, 2, n_steps, [feeds[0], [(0, utt1)]], [p0, p1], [u0, u1], **kw)
    _assert_untouched(a, c, [0])
    assert np.abs(a["pcm"][3:, 0]).max() > 1e-3


# ---- 2. every decode path, device RNG, twin comparison -------------------------------------------------------------------------
CASES = {
    "b2_persistent": dict(B=2, path=1),
    "b3_sampler_edits_multi_launch": dict(B=3, path=0, edits=True),
    "b8_batched_persistent": dict(B=8, path=2),
    "b12_operand_planes": dict(B=12, path=2),
    "b8_fp16_ar": dict(B=8, path=2, fp16=True),
    "b2_chunk4_one_delay_step": dict(B=2, path=1, chunk=4),
    "b2_step_device_pipelined": dict(B=2, path=1, device_steps=True, kw=dict(pipeline=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restart_on_every_decode_path_twin_and_control(eng, eng_fp16, name, record_property):
    cs = CASES[name]
    B, chunk, n_steps = cs["B"], cs.get("chunk", 1), 17
    e = eng_fp16 if cs.get("fp16") else eng
    ua, ub = _utt(7801, 72), _utt(7802, 72)
    pa, pb = _prompt(2801, 107), _prompt(2802, 70)
    last = B - 1
    prompts = [pa if s in (0, last) else pb for s in range(B)]
    seeds = [900 if s in (0, last) else 901 + s for s in range(B)]
    feeds = [[(0, ua)] if s in (0, last) else [(0, ub)] for s in range(B)]
    opt = dict(chunk=chunk, edits=cs.get("edits", False), device_steps=cs.get("device_steps", False), **cs.get("kw", {}))
    ctl = _run(e, B, n_steps, feeds, prompts, seeds, **opt)
    feeds_r = list(feeds)
    feeds_r[last] = [(0, ua), (K0, ua)]
    run = _run(e, B, n_steps, feeds_r, prompts, seeds, events={K0: [("restart", last, pa, 900)]}, **opt)
    assert run["path"] == cs["path"] == ctl["path"], "the case no longer runs the decode path it is named after"
    _assert_untouched(run, ctl, range(B - 1))
    _assert_twin(run, last, K0, chunk=chunk, record_property=record_property)
    np.testing.assert_array_equal(ctl["pcm"][:, 0], ctl["pcm"][:, last])         # (the twins of the control agree to begin with)


# ---- 3. retire ---------------------------------------------------------------------------------------------------------------------
def test_retire_then_restart(eng, record_property):
    B, k_ret, k_re, n_steps = 3, 4, 24, 36
    ua, ub = _utt(7801, 72), _utt(7802, 72)
    pa, pb = _prompt(2801, 107), _prompt(2802, 70)
    prompts, seeds = [pa, pa, pb], [900, 900, 902]
    kw = dict(max_seq_frames=136, buffer_frames=16)            # slots 0 / 2 re-prefill around step 14 / 33, while slot 1 is retired: it never becomes due
    ctl = _run(eng, B, n_steps, [[(0, ua)], [(0, ua)], [(0, ub)]], prompts, seeds, **kw)
    run = _run(eng, B, n_steps, [[(0, ua)], [(0, ua), (k_ret, None), (k_re, ua)], [(0, ub)]], prompts, seeds,
               events={k_ret: [("retire", 1)], k_re: [("restart", 1, pa, 900)]}, **kw)          # (_run ends with sva_sync: no deferred error either)
    assert np.isfinite(run["pcm"]).all()
    assert not run["pcm"][k_ret:k_re + 2, 1].any()             # exact zeros while retired, and while the restarted stream's delay fills
    assert (run["state"][k_ret:k_re, 1] == [0, 0]).all()
    assert np.abs(ctl["pcm"][k_ret:k_re, 1]).max() > 1e-3
    _assert_untouched(run, ctl, [0, 2])
    assert (np.diff(ctl["state"][:, 0, 1]) == 1)[2:].all() and int(ctl["last_pos"][0]) < 33 + 2 * 107 + 3 + 2 * 34      # slot 0 did re-prefill
    assert int(run["last_pos"][1]) == 33 + 2 * 107 - 1 + 3 + 2 * (n_steps - k_re - 2)
    _assert_twin(run, 1, k_re, n_cmp=n_steps - k_re, record_property=record_property)


# ---- 4. two restarts in flight -----------------------------------------------------------------------------------------------------
def test_two_restarts_with_overlapping_delay_phases(eng, record_property):
    B, n_steps = 8, 17
    ua, ub = _utt(7801, 72), _utt(7802, 72)
    pa, pb = _prompt(2801, 107), _prompt(2802, 70)
    twins = (0, 2, 5)
    prompts = [pa if s in twins else pb for s in range(B)]
    seeds = [900 if s in twins else 901 + s for s in range(B)]
    feeds = [[(0, ua)] if s in twins else [(0, ub)] for s in range(B)]
    ctl = _run(eng, B, n_steps, feeds, prompts, seeds)
    feeds_r = list(feeds)
    feeds_r[2], feeds_r[5] = [(0, ua), (5, ua)], [(0, ua), (6, ua)]
    run = _run(eng, B, n_steps, feeds_r, prompts, seeds, events={5: [("restart", 2, pa, 900)], 6: [("restart", 5, pa, 900)]})
    assert run["path"] == 2
    assert run["state"][6, 2, 0] == 2 and run["state"][6, 5, 0] == 1          # slot 2 activates while slot 5 is still filling
    _assert_untouched(run, ctl, [0, 1, 3, 4, 6, 7])
    _assert_twin(run, 2, 5, record_property=record_property, tag="_slot2")
    _assert_twin(run, 5, 6, record_property=record_property, tag="_slot5")


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(eng):
    from streamvoiceanon_amd import engine as E

    ua, ub = _utt(7801, 72), _utt(7802, 72)
    pa, pb = _prompt(2801, 107), _prompt(2802, 70)
    lib = E.load_library()

    def refused(fn, *args):
        with pytest.raises(RuntimeError) as ei:
            fn(*args)
        assert lib.sva_last_error().decode() != "" and lib.sva_last_error().decode() in str(ei.value)

    ctl = _run(eng, 2, 8, [[(0, ua)], [(0, ub)]], [pa, pb], [900, 901])
    b = E.Batch(eng, n_streams=2)
    for s, p in enumerate((pa, pb)):
        b.prefill_prompt(s, p[1], p[0], p[2], p[3], noise_seed=900 + s)
    ac, cc, st, tm = pa
    refused(b.restart, 1, cc, ac, st, tm)                      # before sva_streams_begin
    refused(b.retire, 1)
    refused(b.stream_state, 1)
    b.begin()
    outs = []
    for k in range(8):
        if k == 4:
            refused(b.restart, 2, cc, ac, st, tm)              # slot out of range
            refused(b.restart, -1, cc, ac, st, tm)
            refused(b.retire, 2)
            refused(b.stream_state, 7)
            refused(b.restart, 1, cc[:2], ac[:, :2], st, tm)   # R <= delay
            refused(b.restart, 1, cc[:1], ac[:, :1], st, tm)
            assert b.stream_state(1) == (2, 2)
        outs.append(b.step(np.stack([ua[k * N:(k + 1) * N], ub[k * N:(k + 1) * N]])))
    b.sync()
    np.testing.assert_array_equal(np.stack(outs), ctl["pcm"])
    np.testing.assert_array_equal(b.pred_codes(1), ctl["codes"][1])
    b.close()
    # a configuration without a cached silence state: the full-window encoder of a short encode window
    b = E.Batch(eng, n_streams=1, encode_window_frames=40)
    b.prefill_prompt(0, cc, ac, st, tm)
    b.begin()
    first = b.step(ua[:N])
    refused(b.restart, 0, cc, ac, st, tm)
    assert b.stream_state(0)[0] == 1
    b.retire(0)                                                # retiring needs no encoder state
    assert b.stream_state(0) == (0, 0) and not first.any()
    b.close()


# ---- 6. continuous batching driver -------------------------------------------------------------------------------------------------
def test_stream_infer_many_equals_stream_infer_alone(wrap):
    chunks = (9, 14, 11, 6)
    srcs = [_utt(7810 + u, c)[:N * (c - 1) + 300 + 100 * u] for u, c in enumerate(chunks)]       # stream_infer pads each to c whole chunks
    prompts = [_prompt(2810 + u, (107, 70, 91, 64)[u]) for u in range(4)]
    seeds = [40 + u for u in range(4)]
    alone, alone_codes = [], []
    for u in range(4):
        alone.append(wrap.stream_infer(srcs[u], prompt=prompts[u], noise_seed=seeds[u], save_result=False))
        alone_codes.append(wrap.batch.pred_codes(0))
    codes = [[] for _ in range(4)]
    phases = []

    def on_step(k, feeds):
        t = wrap.batch.tap("audio_codes", (2, 8, 1), np.int32)
        for s, u, i in feeds:
            if i >= 2:
                codes[u].append(t[s, :, 0].copy())
        phases.append([wrap.batch.stream_state(s)[0] for s in range(2)])

    many = wrap.stream_infer_many(srcs, prompts, n_slots=2, noise_seeds=seeds, on_step=on_step)
    assert len(many) == 4 and len(phases) == 20                  # slot 0: 9 + 11 chunks, slot 1: 14 + 6
    for u, c in enumerate(chunks):
        assert many[u].shape == alone[u].shape == (N * c,)
        np.testing.assert_array_equal(np.stack(codes[u], axis=1), alone_codes[u])
        assert not many[u][:2 * N].any() and np.abs(many[u][2 * N:]).max() > 1e-3
        np.testing.assert_allclose(many[u], alone[u], rtol=0, atol=PCM_TOL)
