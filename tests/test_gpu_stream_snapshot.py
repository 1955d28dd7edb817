"""sva_stream_save / sva_stream_load: a live stream leaves its slot as a snapshot and continues somewhere else.

What is pinned (all comparisons exact: a resumed stream runs the same kernels on the same bytes):
  1. resume = uninterrupted, on every decode path: utterance U runs K0 steps in slot 1 of batch A, is saved, and is loaded into slot 0 of a
     landing batch that carries other utterances, is K2 steps old (another ring rotation, another step parity) and was never near U; fed U's
     chunks K0 .. K0 + K1 - 1 it produces the PCM, content codes, audio codes, positions, stream states and code history of the control (U
     uninterrupted in slot 1 of A).  max_seq_frames = 136, buffer_frames = 16 put a re-prefill inside the K1 steps, so the stored prompt and
     both code histories must have travelled.  The landing batch's other slots equal their own control, a run without the load.  Once with
     host steps and taps per path, once with step_device in the pipelined mode;
  2. a save is read-only and deterministic, save_size is what is written and grows by 2 x 73 728 B (2 x 36 864 B with fp16 KV) per frame;
  3. rollback: save, 3 steps, load into the same slot, the same 3 chunks give the same 3 outputs (device RNG);
  4. the sampling pair travels, the target's batch pair does not overwrite it, a later restart puts the batch pair back; loading over a
     retired, a delay-filling restarted and a decoding slot all give the same stream;
  5. every refusal changes nothing: the target's next steps equal its control bit for bit.
Shapes: 2-12 streams, chunk 1, the 107-frame synthetic prompt and synth_utterance sources of tests/test_gpu_stream_restart.py, < 40 steps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N = 2048
K0, K1, K2 = 8, 12, 5            # K2 mod 128 != K0 mod 128 (ring rotations differ), K2 odd / K0 even (parity of the double buffers)
KW = dict(max_seq_frames=136, buffer_frames=16)      # U's slot re-prefills at step 13 (last_pos 249 after the delay fill, + 2 per step, due at 272)
KV_ROW = 12 * 2 * 12 * 64 * 4    # bytes of one KV position in fp32


@pytest.fixture(scope="module")
def eng(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_fp16(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0, ar_dtype=1)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _utt(seed, frames=40):
    from streamvoiceanon_amd.synth_audio import synth_utterance

    a = synth_utterance(seed, N * frames)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _prompt(seed, R=107):
    from streamvoiceanon_amd.synth_audio import synth_prompt

    return synth_prompt(seed, R)          # (ac, cc, style, timbre)


U, PU, SEED_U = 7801, 2801, 900           # the travelling stream: utterance, prompt, noise seed
O, PO = 7802, 2802                        # everybody else


class Rig:
    """One batch stepped chunk by chunk.  feed[slot] = (utterance, first chunk index): the slot reads chunk first + (steps since set_feed)."""

    def __init__(self, engine, B, prompts, seeds, debug=None, device_steps=False, begin=True, **kw):
        from streamvoiceanon_amd import engine as E

        lib = E.load_library()
        if debug:
            lib.sva_debug_configure(debug.encode())          # (read at batch creation)
        try:
            self.b = E.Batch(engine, n_streams=B, **kw)
        finally:
            if debug:
                lib.sva_debug_configure(b"ar_batch=1,ar_persistent=1")
        self.B, self.device_steps, self.chunk = B, device_steps, kw.get("chunk_frames", 1)
        for s in range(B):
            ac, cc, st, tm = prompts[s]
            self.b.prefill_prompt(s, cc, ac, st, tm, noise_seed=seeds[s])
        if begin:
            self.b.begin()
        self.feed = [None] * B
        self.rec = dict(pcm=[], content=[], audio=[], state=[])
        self.path = self.b.decode_path()

    def set_feed(self, slot, utt, first=0):
        self.feed[slot] = [utt, first]

    def steps(self, n):
        b, n_s = self.b, N * self.chunk
        for _ in range(n):
            x = np.zeros((self.B, n_s), np.float32)
            for s, f in enumerate(self.feed):
                if f is not None:
                    x[s] = f[0][f[1] * n_s:(f[1] + 1) * n_s]
                    f[1] += 1
            if self.device_steps:
                din, dout = torch.from_numpy(x).cuda(), torch.zeros(self.B, n_s, device="cuda")
                torch.cuda.synchronize()
                b.step_device(din.data_ptr(), dout.data_ptr())
                b.sync()
                self.rec["pcm"].append(dout.cpu().numpy())
            else:
                self.rec["pcm"].append(b.step(x))
                self.rec["content"].append(b.tap("content_codes", (self.B, self.chunk), np.int32).copy())
                self.rec["audio"].append(b.tap("audio_codes", (self.B, 8, self.chunk), np.int32).copy())
            self.rec["state"].append([b.stream_state(s) for s in range(self.B)])
        return self

    def finish(self):
        b = self.b
        b.sync()                                            # raises on any deferred error
        r = {k: np.stack(v) for k, v in self.rec.items() if v}
        r["codes"] = [b.pred_codes(s) if b.frames_decoded(s) else np.zeros((8, 0), np.int32) for s in range(self.B)]
        r["last_pos"] = b.tap("last_pos", (self.B,), np.int32).copy()
        r["path"] = self.path
        b.close()
        return r


def _source(engine, B, slot=1, **opt):
    """batch A: U in `slot`, the other utterance everywhere else"""
    rig = Rig(engine, B, [_prompt(PU) if s == slot else _prompt(PO, 70) for s in range(B)], [SEED_U if s == slot else 901 + s for s in range(B)], **opt)
    for s in range(B):
        rig.set_feed(s, _utt(U) if s == slot else _utt(O))
    return rig


def _landing(engine, B, **opt):
    """batch D: other utterances in every slot"""
    rig = Rig(engine, B, [_prompt(PO + 1 + s % 2, 70) for s in range(B)], [950 + s for s in range(B)], **opt)
    for s in range(B):
        rig.set_feed(s, _utt(O + 1 + s % 3))
    return rig


def _assert_slot_equal(got, g_slot, g0, want, w_slot, w0, n, what):
    """steps g0 .. g0 + n of slot g_slot of `got` = steps w0 .. w0 + n of slot w_slot of `want`"""
    np.testing.assert_array_equal(got["pcm"][g0:g0 + n, g_slot], want["pcm"][w0:w0 + n, w_slot], err_msg=f"pcm: {what}")
    np.testing.assert_array_equal(got["state"][g0:g0 + n, g_slot], want["state"][w0:w0 + n, w_slot], err_msg=f"stream_state: {what}")
    if "content" in got:
        np.testing.assert_array_equal(got["content"][g0:g0 + n, g_slot], want["content"][w0:w0 + n, w_slot], err_msg=f"content codes: {what}")
        np.testing.assert_array_equal(got["audio"][g0:g0 + n, g_slot], want["audio"][w0:w0 + n, w_slot], err_msg=f"audio codes: {what}")


# ---- 1. resume = uninterrupted, on every decode path -----------------------------------------------------------------------------------
CASES = {
    "b3_persistent": dict(B=3, path=1),
    "b8_batched_persistent": dict(B=8, path=2),
    "b3_multi_launch": dict(B=3, path=0, debug="ar_persistent=0"),
    "b8_fp16_kv": dict(B=8, path=2, fp16=True),
    "b12_operand_planes": dict(B=12, path=2),
    "b3_step_device_pipelined": dict(B=3, path=1, device_steps=True, kw=dict(pipeline=True)),
    "b8_step_device_pipelined": dict(B=8, path=2, device_steps=True, kw=dict(pipeline=True)),
    "b12_step_device_pipelined_planes": dict(B=12, path=2, device_steps=True, kw=dict(pipeline=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_resume_equals_uninterrupted(eng, eng_fp16, name):
    cs = CASES[name]
    B, e = cs["B"], eng_fp16 if cs.get("fp16") else eng
    opt = dict(debug=cs.get("debug"), device_steps=cs.get("device_steps", False), **KW, **cs.get("kw", {}))
    ctl = _source(e, B, **opt).steps(K0 + K1).finish()
    assert ctl["path"] == cs["path"], "the case no longer runs the decode path it is named after"
    # U re-prefills inside the K1 steps after the save: its position falls back, once
    assert (np.diff(ctl["state"][2:, 1, 1]) == 1).all() and int(ctl["last_pos"][1]) < 249 + 2 * (K0 + K1 - 2) and ctl["state"][K0 - 1, 1, 1] == K0 - 2
    src = _source(e, B, **opt).steps(K0)
    blob = src.b.save_stream(1)
    if cs.get("device_steps"):            # the source was in the pipelined regime when it was saved (the first steady steps of a batch run eagerly)
        src_pipe = src.b.snapshot_timings()["pipelined_steps"]
        assert src_pipe >= 3
    src.finish()
    land_ctl = _landing(e, B, **opt).steps(K2 + K1).finish()
    land = _landing(e, B, **opt).steps(K2)
    assert land.path == cs["path"]
    if cs.get("device_steps"):            # ... and so was the landing batch, on the other parity of its double buffers
        n_pipe = land.b.snapshot_timings()["pipelined_steps"]
        assert n_pipe >= 1 and (n_pipe - src_pipe) % 2 == 1
    land.b.load_stream(0, blob)
    land.set_feed(0, _utt(U), K0)
    land.steps(K1)
    if cs.get("device_steps"):
        assert land.b.snapshot_timings()["pipelined_steps"] == n_pipe + K1
    got = land.finish()
    _assert_slot_equal(got, 0, K2, ctl, 1, K0, K1, "resumed slot vs the uninterrupted control")
    np.testing.assert_array_equal(got["codes"][0], ctl["codes"][1], err_msg="pred_codes of the resumed slot (the whole stream's frames)")
    assert int(got["last_pos"][0]) == int(ctl["last_pos"][1])
    assert np.abs(got["pcm"][K2:, 0]).max() > 1e-3
    for s in range(1, B):
        _assert_slot_equal(got, s, 0, land_ctl, s, 0, K2 + K1, f"slot {s} of the landing batch vs a run without the load")
        np.testing.assert_array_equal(got["codes"][s], land_ctl["codes"][s])
    np.testing.assert_array_equal(got["last_pos"][1:], land_ctl["last_pos"][1:])


# ---- 2. save is read-only and deterministic --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32_kv", "fp16_kv"])
def test_save_is_read_only_and_deterministic(eng, eng_fp16, fp16):
    from streamvoiceanon_amd import engine as E

    e, B = (eng_fp16 if fp16 else eng), 3
    ctl = _source(e, B).steps(K0 + 4).finish()
    run = _source(e, B).steps(K0)
    n0 = run.b.save_size(1)
    a, b_ = run.b.save_stream(1), run.b.save_stream(1)
    assert a == b_ and len(a) == n0 == run.b.save_size(1)
    info = E.stream_blob_info(a)
    assert (info["frames"], info["last_pos"], info["ncontent"], info["ref_len"]) == (K0 - 2, 249 + 2 * (K0 - 2), K0, 107)
    assert info["ar_dtype"] == int(fp16) and info["chunk_frames"] == 1 and info["version"] == 1
    run.steps(4)
    n1 = run.b.save_size(1)
    c = run.b.save_stream(1)
    assert len(c) == n1 == n0 + 4 * 2 * (KV_ROW // 2 if fp16 else KV_ROW)          # two KV positions per decoded frame, nothing else grows
    got = run.finish()
    for s in range(B):
        _assert_slot_equal(got, s, 0, ctl, s, 0, K0 + 4, f"slot {s} of a batch that was saved from vs its control")
        np.testing.assert_array_equal(got["codes"][s], ctl["codes"][s])
    np.testing.assert_array_equal(got["last_pos"], ctl["last_pos"])


# ---- 3. rollback -----------------------------------------------------------------------------------------------------------------------
def test_rollback_into_the_same_slot(eng):
    B = 3
    ctl = _source(eng, B).steps(K0 + 6).finish()
    run = _source(eng, B).steps(K0)
    blob = run.b.save_stream(1)
    run.steps(3)
    run.b.load_stream(1, blob)
    run.set_feed(1, _utt(U), K0)                   # the same three chunks again
    got = run.steps(3).finish()
    _assert_slot_equal(got, 1, K0 + 3, got, 1, K0, 3, "the three steps after the rollback vs the three before it")
    _assert_slot_equal(got, 1, K0 + 3, ctl, 1, K0, 3, "... and vs the control")
    for s in (0, 2):
        _assert_slot_equal(got, s, 0, ctl, s, 0, K0 + 6, f"slot {s} beside the rollback")
    assert got["codes"][1].shape[1] == K0 + 3 - 2 and int(got["last_pos"][1]) == int(ctl["last_pos"][1]) - 6


# ---- 4. what travels and what does not -------------------------------------------------------------------------------------------------
def test_sampling_pair_travels_and_any_phase_is_a_landing_slot(eng):
    B, f32 = 3, lambda v: float(np.float32(v))
    pair = (0.9, 0.5)

    def source(n):
        rig = _source(eng, B)
        rig.b.set_sampling(1, *pair)
        return rig.steps(n)

    ctl = source(K0 + 6).finish()
    src = source(K0)
    blob = src.b.save_stream(1)
    src.finish()
    land = _landing(eng, B, temperature=0.6, top_p=0.8).steps(K2)
    land.b.retire(1)
    ac, cc, st, tm = _prompt(PO, 70)
    land.b.restart(2, cc, ac, st, tm, noise_seed=5)
    land.steps(1)                                   # slot 2 is filling its own delay now
    assert [land.b.stream_state(s)[0] for s in range(B)] == [2, 0, 1]
    for s in range(B):
        land.b.load_stream(s, blob)
        land.set_feed(s, _utt(U), K0)
        assert land.b.stream_state(s) == (2, K0 - 2)
        assert land.b.sampling(s) == (f32(pair[0]), f32(pair[1]))          # the blob's pair, not the landing batch's
    got_rig = land.steps(6)
    land.b.restart(0, cc, ac, st, tm, noise_seed=6)
    assert land.b.sampling(0) == (f32(0.6), f32(0.8))                      # a restart puts the batch's pair back
    assert land.b.sampling(1) == (f32(pair[0]), f32(pair[1]))
    got = got_rig.finish()
    for s in range(B):
        _assert_slot_equal(got, s, K2 + 1, ctl, 1, K0, 6, f"slot {s} (loaded over phase {[2, 0, 1][s]}) vs the source's control")
        np.testing.assert_array_equal(got["codes"][s], ctl["codes"][1])
    assert np.abs(got["pcm"][K2 + 1:]).max() > 1e-3
    # the pair matters: without it the source decodes other frames
    plain = _source(eng, B).steps(K0 + 6).finish()
    assert not np.array_equal(plain["codes"][1], ctl["codes"][1])


# ---- 6. server: SAVE on one connection, LOAD on the next ----------------------------------------------------------------------------------
def test_server_save_then_load_on_a_new_connection(weights0):
    import threading

    from streamvoiceanon_amd import stream_server as S
    from streamvoiceanon_amd.infer_arvc import InferenceWrapper
    from streamvoiceanon_amd.realtime import RealtimeSession
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

    _, _, style, timbre = synth_prompt(2500, 8)
    ref, src = synth_utterance(7300, N * 70 + 100), synth_utterance(7302, N * 12)
    prefills = []

    def make(count):
        w = InferenceWrapper(weights=weights0)
        w.style_encoder = lambda wav: style
        w.timbre_encoder = lambda wav: timbre
        if count:
            orig = w.prefill_prompt
            w.prefill_prompt = lambda *a, **k: (prefills.append(1), orig(*a, **k))[1]
        return w

    w_srv, ready = make(True), threading.Event()
    th = threading.Thread(target=S.serve, args=(w_srv, "127.0.0.1", 0, 3, ready), daemon=True)
    th.start()
    assert ready.wait(30)
    blocks = [src[i * N:(i + 1) * N] for i in range(12)]
    c = S.Client(port=ready.port)
    c.configure(alpha=1.0, block_frame=1, n_frame_delay=2)
    c.set_reference("a.wav", ref)
    with pytest.raises(RuntimeError, match="no stream yet"):
        c.save()                                              # nothing to save before the first block
    first = [c.convert(x) for x in blocks[:6]]
    env = c.save()
    c.close()
    assert len(prefills) == 1
    c = S.Client(port=ready.port)                             # a new connection = a new session: no REF, the envelope carries the stream
    c.configure(alpha=1.0, block_frame=1, n_frame_delay=2)
    with pytest.raises(RuntimeError, match="envelope"):
        c.load(env[:10])
    with pytest.raises(RuntimeError, match="truncated"):
        c.load(env[:-32])
    c.load(env)
    rest = [c.convert(x) for x in blocks[6:]]
    c.configure_io(sample_rate=48000, fmt=0, max_block=4096)
    with pytest.raises(RuntimeError, match="IOCONF"):
        c.save()
    with pytest.raises(RuntimeError, match="IOCONF"):
        c.load(env)
    c.close()
    assert len(prefills) == 1, "the loaded session re-prefilled its prompt"
    c = S.Client(port=ready.port)                             # the same twelve blocks on one uninterrupted connection
    c.configure(alpha=1.0, block_frame=1, n_frame_delay=2)
    c.set_reference("a.wav", ref)
    want = [c.convert(x) for x in blocks]
    c.close()
    th.join(30)
    assert len(prefills) == 2
    np.testing.assert_array_equal(np.stack(first + rest), np.stack(want))
    assert not np.stack(want)[:2].any() and np.abs(np.stack(want)[6:]).max() > 1e-3
    # in process, into a wrapper that has no batch at all: the landing batch comes from engine.idle_batch
    w2, sess = make(False), RealtimeSession()
    assert sess.load(w2, env) == ("a.wav", 1, 2)
    got = [sess.custom_infer(w2, None, "a.wav", x, n_frame_delay=2, alpha=1.0) for x in blocks[6:]]
    assert sess.prefills == 0
    np.testing.assert_array_equal(np.stack(got), np.stack(want[6:]))
    w_srv.engine.close(); w2.engine.close()


# ---- 5. refusals change nothing --------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(eng, eng_fp16):
    import ctypes as C

    from streamvoiceanon_amd import engine as E

    lib = E.load_library()

    def refused(match, fn, *args):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*args)
        assert lib.sva_last_error().decode() in str(ei.value)

    def blob_of(engine, B=2, steps=4, **kw):
        rig = _source(engine, B, **kw).steps(steps)
        blob = rig.b.save_stream(1)
        rig.finish()
        return blob

    good = blob_of(eng, **KW)
    B, n = 2, 9
    ctl = _landing(eng, B, **KW).steps(n).finish()
    # before begin, and before the lock-step delay has filled
    run = _landing(eng, B, begin=False, **KW)
    refused("not begun", run.b.save_stream, 0)
    refused("not begun", run.b.load_stream, 0, good)
    refused("not begun", run.b.save_size, 0)
    run.b.begin()
    refused("delay has not filled", run.b.load_stream, 0, good)
    refused("phase 2", run.b.save_stream, 0)                     # a slot that is still filling its delay
    run.steps(4)
    run_slot1 = run.b.save_stream(1)
    refused("slot out of range", run.b.load_stream, B, good)
    refused("slot out of range", run.b.load_stream, -1, good)
    refused("slot out of range", run.b.save_stream, B)
    refused("truncated", run.b.load_stream, 0, good[:-16])
    refused("truncated", run.b.load_stream, 0, good[:60])
    refused("truncated", run.b.load_stream, 0, b"")
    info = E.stream_blob_info(good)
    hb = len(good) - info["payload_bytes"]
    for i, match in ((hb + 12345, "payload fails its checksum"), (70, "header is corrupt"), (3, "wrong magic"), (8, "format version")):
        bad = bytearray(good)
        bad[i] ^= 0x04
        refused(match, run.b.load_stream, 0, bytes(bad))
    # a blob whose checksums are right but whose code tables would index outside the embedding tables (rebuilt through the container hook,
    # which computes both checksums): the stored prompt in the header, the content history in the payload
    cfg_n, lay_n = int.from_bytes(good[48:52], "little"), int.from_bytes(good[52:56], "little")
    sig = np.frombuffer(good[104:104 + 8 * (cfg_n + lay_n)], "<i8")
    cfg_sig, lay_sig = sig[:cfg_n], sig[cfg_n:]
    o = 104 + 8 * (cfg_n + lay_n)
    cc = np.frombuffer(good[o:o + 8 * 107], "<i8").copy()
    ac = np.frombuffer(good[o + 8 * 107:o + 8 * 107 + 4 * 8 * 107], "<i4").reshape(8, 107).astype(np.int64)
    fields = (info["frames"], info["last_pos"], info["ncontent"], 0, 1)
    payload = bytearray(good[hb:])
    rebuilt = E.test_snapshot_build(cfg_sig, lay_sig, fields, cc, ac, bytes(payload))
    assert rebuilt[hb:] == good[hb:] and E.stream_blob_info(rebuilt) == info
    off = 0
    for rows, row_bytes, kind in lay_sig[:3 * ((lay_n - 10) // 3)].reshape(-1, 3):
        if (rows, row_bytes, kind) == (1, 4 * 4096, 0):
            break                                                # the first [hist_cap] int32 ring of the inventory: d_content_hist
        off += ((info["last_pos"] + 1 if kind == 2 else rows) * row_bytes + 15) // 16 * 16
    payload[off + 8:off + 12] = (8192).to_bytes(4, "little")     # ar_vocab: one past the content embedding table
    refused("d_content_hist is outside its embedding table", run.b.load_stream, 0, E.test_snapshot_build(cfg_sig, lay_sig, fields, cc, ac, bytes(payload)))
    bad_cc = cc.copy()
    bad_cc[5] = -1
    refused("slot field is out of range", run.b.load_stream, 0, E.test_snapshot_build(cfg_sig, lay_sig, fields, bad_cc, ac, good[hb:]))
    bad_ac = ac.copy()
    bad_ac[7, 106] = 1000
    refused("slot field is out of range", run.b.load_stream, 0, E.test_snapshot_build(cfg_sig, lay_sig, fields, cc, bad_ac, good[hb:]))
    for f_bad in ((info["frames"], 100, info["ncontent"], 0, 1), (info["ncontent"], info["last_pos"], info["ncontent"], 0, 1)):      # position inside the prompt; more frames than codes
        refused("slot field is out of range", run.b.load_stream, 0, E.test_snapshot_build(cfg_sig, lay_sig, f_bad, cc, ac, good[hb:]))
    run.b.load_stream(1, rebuilt)                                # (the rebuilt blob itself is a good one ...
    run.b.load_stream(1, run_slot1)                              #  ... and slot 1 gets its own stream back)
    # a buffer that is too small: *written = needed, nothing written
    need = run.b.save_size(0)
    small, wr = np.full(1024, 0xEE, np.uint8), C.c_long(0)
    assert lib.sva_stream_save(run.b.h, 0, small.ctypes.data_as(C.c_void_p), small.size, C.byref(wr)) != 0
    assert wr.value == need and (small == 0xEE).all() and "smaller than the snapshot" in lib.sva_last_error().decode()
    refused(r"configuration differs.*\(chunk_frames\)", run.b.load_stream, 0, blob_of(eng, chunk_frames=2, **KW))
    refused(r"configuration differs.*\(ar_dtype\)", run.b.load_stream, 0, blob_of(eng_fp16, **KW))
    refused(r"configuration differs.*\(max_seq_frames\)", run.b.load_stream, 0, blob_of(eng, max_seq_frames=200, buffer_frames=16))
    refused(r"layout differs.*first differing field \d+ \(", run.b.load_stream, 0, blob_of(eng, B=12, **KW))      # a planes-form batch's vocoder state
    io = run.b.open_io(44100)
    refused("I/O adaptor", run.b.load_stream, 0, good)
    refused("I/O adaptor", run.b.save_stream, 0)
    io.close()
    run.b.retire(1)
    refused("phase 2", run.b.save_stream, 1)                     # a retired slot is no source
    assert [run.b.stream_state(s)[0] for s in range(B)] == [2, 0]
    got = run.steps(n - 4).finish()
    _assert_slot_equal(got, 0, 0, ctl, 0, 0, n, "slot 0 of the target after every refused call vs its control")
    _assert_slot_equal(got, 1, 0, ctl, 1, 0, 4, "slot 1 up to its retirement")
    np.testing.assert_array_equal(got["codes"][0], ctl["codes"][0])
    # a batch whose persistent kernel has timed out refuses both (the timeout word is written by the test hook: nothing hangs)
    rig = _source(eng, 2, **KW).steps(3)
    assert rig.path == 1 and lib.sva_test_force_ar_timeout(rig.b.h) == 0
    with pytest.raises(RuntimeError, match="timed out"):
        rig.b.sync()
    refused("timed out", rig.b.save_stream, 1)
    refused("timed out", rig.b.load_stream, 0, good)
    rig.b.close()
