"""The I/O adaptor (include/sva.h: sva_io_*; csrc/io/): a batch fed and read at a caller-chosen sample rate, in blocks of any length, as
float32 or int16, with everything between the caller's buffer and the engine's 44.1 kHz chunk on the device.

Kernel level, through sva_test_resample (engine.test_resample), both kernels in the directions 48 k, 16 k and 8 k <-> 44.1 k:
  * against the float64 evaluation of audio_io.resample's sum, every sample of resample()'s own output length, within the derived bound
    (taps + 1) * 2^-24 * sum|k_p| * max|x| per output: taps + 1 roundings of relative size 2^-24 -- the weight's rounding to fp32 and the
    fmaf of each tap -- each on a magnitude of at most sum|k_p| * max|x|;
  * bit-identical however the input is cut into calls;
  * int16 on either side equals the float path's conversion exactly, saturation included.
End to end on a two-stream batch: the adaptor returns, bit for bit, L zeros followed by the resampled output of a plain twin batch that was
stepped with the resampled input; block length and the pipelined mode change nothing; 44.1 kHz is a pure delay; retire / restart of one slot
leave the other one bit-identical; refusals change nothing; the server's IOCONF frame reaches the same adaptor."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MODEL = 44100
DIRECTIONS = [(48000, MODEL), (MODEL, 48000), (16000, MODEL), (MODEL, 16000), (8000, MODEL), (MODEL, 8000)]


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(fr, to):
    """signal [2][3 * orig + 2 * taps + 37] (impulses at both ends | seeded noise in [-1, 1]) padded with the zeros resample() pads with,
    its float64 resampling and the bound per output"""
    from streamvoiceanon_amd import audio_io

    g = math.gcd(fr, to)
    orig, new = fr // g, to // g
    kern, width = audio_io._sinc_resample_kernel(orig, new)
    taps = kern.shape[1]
    n = 3 * orig + 2 * taps + 37
    x = np.zeros((2, n), np.float32)
    x[0, 0], x[0, -1] = 1.0, -1.0
    x[1] = np.random.default_rng(fr + to).uniform(-1.0, 1.0, n).astype(np.float32)
    padded = np.pad(x.astype(np.float64), ((0, 0), (width, width + orig)))
    n_blocks = (padded.shape[1] - taps) // orig + 1
    frames = np.lib.stride_tricks.sliding_window_view(padded, taps, axis=1)[:, ::orig][:, :n_blocks]
    target = int(math.ceil(new * n / orig))
    ref = (frames @ kern.T).reshape(2, -1)[:, :target]
    bound = (taps + 1) * 2.0 ** -24 * np.abs(kern).sum(axis=1)[np.arange(target) % new] * np.abs(x).max()
    xpad = np.pad(x, ((0, 0), (0, width + orig)))
    for a in (xpad, ref, bound):
        a.setflags(write=False)
    return xpad, ref, bound, target


def _splits(n, kind):
    if kind == "none":
        return []
    if kind == "every":
        return list(range(1, n))
    if kind == "480":
        return list(range(480, n, 480))
    rng = np.random.default_rng(n)
    cuts, at = [], 0
    while True:
        at += int(rng.integers(1, 700))
        if at >= n:
            return cuts
        cuts.append(at)


@functools.lru_cache(maxsize=None)
def _whole(fr, to):
    from streamvoiceanon_amd import engine as E

    y = E.test_resample(_case(fr, to)[0], fr, to)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("fr,to", DIRECTIONS)
def test_resample_matches_fp64(fr, to):
    xpad, ref, bound, target = _case(fr, to)
    y = _whole(fr, to)
    assert y.shape[1] >= target, "the zeros resample() pads with make every sample of its output ready"
    err = np.abs(y[:, :target].astype(np.float64) - ref)
    print(f"{fr} -> {to}: {target} samples, max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.abs(ref[1]).max() > 0.3 and np.abs(ref[0]).max() > 0.05
    assert (err <= bound).all(), f"max err / bound {np.max(err / bound):.3f} at {np.unravel_index(np.argmax(err / bound), err.shape)}"


@pytest.mark.parametrize("kind", ["every", "480", "ragged"])
@pytest.mark.parametrize("fr,to", DIRECTIONS)
def test_resample_is_independent_of_the_block_split(fr, to, kind):
    from streamvoiceanon_amd import engine as E

    xpad = _case(fr, to)[0]
    y = E.test_resample(xpad, fr, to, splits=_splits(xpad.shape[1], kind))
    np.testing.assert_array_equal(y.view(np.int32), _whole(fr, to).view(np.int32))


def _to_i16(y):
    """round to nearest even of y * 32768 (exact in fp32: a power of two), saturated"""
    return np.clip(np.rint(y.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("to", [48000, 16000, 8000])
def test_int16_output_is_the_rounded_saturated_float_path(to):
    from streamvoiceanon_amd import engine as E

    n = _case(MODEL, to)[0].shape[1]
    x = np.where(np.random.default_rng(to).integers(0, 2, (2, n)) > 0, 1.0, -1.0).astype(np.float32)      # full scale: the filter overshoots
    cuts = _splits(n, "ragged")
    yf = E.test_resample(x, MODEL, to, splits=cuts)
    yi = E.test_resample(x, MODEL, to, splits=cuts, fmt_out="i16")
    assert yi.dtype == np.int16
    np.testing.assert_array_equal(yi, _to_i16(yf))
    if to == 48000:
        assert (yi == 32767).any() and (yi == -32768).any() and (np.abs(yf) > 1.0).any(), "the saturation is exercised"


@pytest.mark.parametrize("fr", [48000, 16000, 8000])
def test_int16_input_is_x_over_32768(fr):
    from streamvoiceanon_amd import engine as E

    n = _case(fr, MODEL)[0].shape[1]
    xi = np.random.default_rng(fr).integers(-32768, 32768, (2, n)).astype(np.int16)
    xi[0, :2] = (-32768, 32767)
    cuts = _splits(n, "480")
    yi = E.test_resample(xi, fr, MODEL, splits=cuts, fmt_in="i16")
    yf = E.test_resample(xi.astype(np.float32) / np.float32(32768.0), fr, MODEL, splits=cuts)
    np.testing.assert_array_equal(yi.view(np.int32), yf.view(np.int32))


def test_int16_identity_at_44100():
    from streamvoiceanon_amd import engine as E

    xi = np.random.default_rng(44100).integers(-32768, 32768, (2, 5000)).astype(np.int16)
    xi[1, :2] = (-32768, 32767)
    np.testing.assert_array_equal(E.test_resample(xi, MODEL, MODEL, splits=_splits(5000, "ragged"), fmt_in="i16", fmt_out="i16"), xi)
    xf = np.random.default_rng(1).standard_normal((2, 3000)).astype(np.float32)
    xf[0, :3] = (-0.0, np.float32(1e-42), np.inf)           # copied, not filtered: the bits survive
    np.testing.assert_array_equal(E.test_resample(xf, MODEL, MODEL, splits=[1, 2, 1000]).view(np.int32), xf.view(np.int32))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
B = 2
SEEDS = (4100, 4101)
BATCH_KW = dict(n_streams=B, chunk_frames=1, encode_window_frames=64)
N48 = 480 * 38            # 8 chunks' worth of 48 kHz input (8 * 2048 * 160 / 147 = 17833) and the look-ahead of the last one


@pytest.fixture(scope="module")
def eng(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _prompt(seed):
    from streamvoiceanon_amd.synth_audio import synth_prompt

    return synth_prompt(seed, 107)          # (ac, cc, style, timbre)


@functools.lru_cache(maxsize=None)
def _source(n):
    from streamvoiceanon_amd.synth_audio import synth_utterance

    x = np.stack([synth_utterance(7700 + s, n) for s in range(B)]).astype(np.float32)
    x.setflags(write=False)
    return x


def _batch(eng, **kw):
    from streamvoiceanon_amd import engine as E

    b = E.Batch(eng, **{**BATCH_KW, **kw})
    for s in range(B):
        ac, cc, st, tm = _prompt(2000 + s)
        b.prefill_prompt(s, cc, ac, st, tm, noise_seed=SEEDS[s])
    b.begin()
    return b


def _adaptor_run(eng, x, io_rate, block, fmt="f32", events=None, **kw):
    """x [B][n] through an adaptor in calls of `block` samples; events[i] = what happens before call i: ("retire", slot),
    ("restart", slot, prompt seed, noise seed), ("refusals",)"""
    b = _batch(eng, **kw)
    io = b.open_io(io_rate, fmt, max_block=max(block, 2229))
    out, steps = [], 0
    for i, at in enumerate(range(0, x.shape[1], block)):
        for ev in (events or {}).get(i, ()):
            if ev[0] == "retire":
                b.retire(ev[1])
            elif ev[0] == "restart":
                ac, cc, st, tm = _prompt(ev[2])
                b.restart(ev[1], cc, ac, st, tm, noise_seed=ev[3])
            else:
                with pytest.raises(RuntimeError, match="adaptor is open"):
                    b.step(np.zeros((B, 2048), np.float32))
                with pytest.raises(RuntimeError, match="adaptor is open"):
                    b.stream_chunks(np.zeros((B, 2048), np.float32))
                with pytest.raises(RuntimeError, match="max_block"):
                    io.process(np.zeros((B, io.max_block + 1), io.dtype))
        out.append(io.process(x[:, at:at + block]))
        steps += io.steps_run
    b.sync()
    rec = dict(out=np.concatenate(out, axis=1), steps=steps, L=io.latency, codes=[b.pred_codes(s) for s in range(B)])
    io.close()
    b.step(np.zeros((B, 2048 * b.chunk), np.float32))      # a closed adaptor gives the batch back
    b.close()
    return rec


@pytest.fixture(scope="module")
def run48(eng):
    return _adaptor_run(eng, _source(2229 * 9)[:, :N48], 48000, 480)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def test_adaptor_equals_a_plain_twin_fed_the_resampled_signal(eng, run48):
    from streamvoiceanon_amd import engine as E

    x = _source(2229 * 9)[:, :N48]
    X = E.test_resample(x, 48000, MODEL)
    n_steps = X.shape[1] // 2048
    assert n_steps == run48["steps"] == 8
    twin = _batch(eng)
    Y = np.concatenate([twin.step(X[:, k * 2048:(k + 1) * 2048]) for k in range(n_steps)], axis=1)
    codes = [twin.pred_codes(s) for s in range(B)]
    twin.close()
    y = E.test_resample(Y, MODEL, 48000)
    want = np.concatenate([np.zeros((B, run48["L"]), np.float32), y], axis=1)
    assert want.shape[1] >= N48, "L is large enough for every call to pop what it pushed"
    np.testing.assert_array_equal(_bits(run48["out"]), _bits(want[:, :N48]))
    for s in range(B):
        np.testing.assert_array_equal(run48["codes"][s], codes[s])
        assert codes[s].shape[1] >= 4 and np.abs(run48["out"][s]).max() > 1e-3          # (delay 2: the decoded frames are in the output)
    head, _ = E.test_io_plan(48000, 1, [480])
    assert run48["L"] == head["L"]


@pytest.mark.parametrize("variant", ["blocks of 2229", "pipeline"])
def test_block_length_and_pipelining_change_nothing(eng, run48, variant):
    if variant == "pipeline":
        run = _adaptor_run(eng, _source(2229 * 9)[:, :N48], 48000, 480, pipeline=True)
    else:
        run = _adaptor_run(eng, _source(2229 * 9), 48000, 2229)
    np.testing.assert_array_equal(_bits(run["out"][:, :N48]), _bits(run48["out"]))
    for s in range(B):
        n = min(run["codes"][s].shape[1], run48["codes"][s].shape[1])
        assert n >= 6
        np.testing.assert_array_equal(run["codes"][s][:, :n], run48["codes"][s][:, :n])


@pytest.mark.parametrize("io_rate,fmt,big,small,chunk,n_big", [(8000, "i16", 480, 80, 1, 8), (16000, "f32", 960, 320, 4, 16)])
def test_calls_that_run_several_steps_or_none(eng, io_rate, fmt, big, small, chunk, n_big):
    """8 kHz in 60 ms blocks: a call makes 2646 model-rate samples ready and runs one or two steps; 4-frame chunks at 16 kHz: most calls run
    none.  Either way the result is the one of the same samples in small blocks, and the steps are the planner's."""
    from streamvoiceanon_amd import engine as E

    x = _source(2229 * 9)[:, :big * n_big]
    if fmt == "i16":
        x = _to_i16(x)
    runs = [_adaptor_run(eng, x, io_rate, blk, fmt=fmt, chunk_frames=chunk) for blk in (big, small)]
    _, rows = E.test_io_plan(io_rate, chunk, [big] * n_big)
    assert runs[0]["steps"] == runs[1]["steps"] == rows[:, 1].sum()
    assert rows[:, 1].max() == 2 if chunk == 1 else rows[:, 1].min() == 0
    assert runs[0]["out"].dtype == x.dtype
    np.testing.assert_array_equal(_bits(runs[0]["out"]), _bits(runs[1]["out"]))
    for s in range(B):
        np.testing.assert_array_equal(runs[0]["codes"][s], runs[1]["codes"][s])
        assert runs[0]["codes"][s].shape[1] >= chunk and np.abs(runs[0]["out"][s].astype(np.float32)).max() > (30 if fmt == "i16" else 1e-3)


def test_pass_through_at_44100_is_a_pure_delay(eng):
    x = _source(2229 * 9)[:, :18000]
    run = _adaptor_run(eng, x, MODEL, 1000)
    L = run["L"]
    assert L == 2047 and run["steps"] == 8
    plain = _batch(eng)
    Y = plain.stream_chunks(x[:, :8 * 2048])
    plain.close()
    assert not run["out"][:, :L].any()
    np.testing.assert_array_equal(_bits(run["out"][:, L:]), _bits(Y[:, :18000 - L]))
    assert np.abs(Y).max() > 1e-3


def test_retired_slot_is_silent_and_reads_nothing(eng, run48):
    x = _source(2229 * 9)[:, :N48].copy()
    i_ret = 25
    x[1, 480 * i_ret:] = np.nan
    run = _adaptor_run(eng, x, 48000, 480, events={i_ret: [("retire", 1)]})
    np.testing.assert_array_equal(_bits(run["out"][0]), _bits(run48["out"][0]))
    np.testing.assert_array_equal(run["codes"][0], run48["codes"][0])
    assert np.isfinite(run["out"]).all()
    # what the slot produced before it retired leaves through the FIFO (L samples) and the output filter's history (161 taps at 44.1 kHz)
    tail = 480 * i_ret + run["L"] + 200
    np.testing.assert_array_equal(_bits(run["out"][1, :480 * i_ret]), _bits(run48["out"][1, :480 * i_ret]))
    assert tail < N48 - 1000 and not run["out"][1, tail:].any()


def test_restarted_slot_is_a_fresh_slot_fed_zeros(eng, run48):
    """Restart slot 1 in the middle of a chunk.  Everything it received before counts as zeros: the run equals one in which the slot was
    restarted a call earlier -- no engine step lies between the two points -- and fed zeros up to the restart point."""
    from streamvoiceanon_amd import engine as E

    _, rows = E.test_io_plan(48000, 1, [480] * 38)
    i_r = 12
    assert rows[i_r - 1, 1] == 0 and rows[i_r - 1, 3] > 480 * 147 // 160 > 0, "call i_r - 1 runs no step and leaves its samples staged"
    x = _source(2229 * 9)[:, :N48]
    run = _adaptor_run(eng, x, 48000, 480, events={i_r: [("restart", 1, 2007, 4107)]})
    np.testing.assert_array_equal(_bits(run["out"][0]), _bits(run48["out"][0]))
    np.testing.assert_array_equal(run["codes"][0], run48["codes"][0])
    x0 = x.copy()
    x0[1, 480 * (i_r - 1):480 * i_r] = 0.0
    fresh = _adaptor_run(eng, x0, 48000, 480, events={i_r - 1: [("restart", 1, 2007, 4107)]})
    np.testing.assert_array_equal(_bits(run["out"][1]), _bits(fresh["out"][1]))
    np.testing.assert_array_equal(run["codes"][1], fresh["codes"][1])
    assert run["codes"][1].shape[1] >= 2 and np.abs(run["out"][1, 480 * i_r + run["L"] + 3 * 2229:]).max() > 1e-3
    assert not np.array_equal(run["out"][1], run48["out"][1])
    # ... and directly: a plain twin batch stepped with the resampled signal, slot 1's samples before the restart point replaced by zeros, and
    # restarted at the step boundary the restart fell behind.  What the old stream had already put into the output FIFO (the output samples
    # of the steps before) still leaves; everything later is the twin's output resampled, with the steps before the restart as zeros.
    k0, r0 = int(rows[:i_r, 1].sum()), int(rows[:i_r, 2].sum())
    xz = x.copy()
    xz[1, :480 * i_r] = 0.0
    X = E.test_resample(xz, 48000, MODEL)
    n_steps = X.shape[1] // 2048
    assert n_steps == run["steps"] and 0 < k0 < n_steps
    twin = _batch(eng)
    Y = []
    for k in range(n_steps):
        if k == k0:
            ac, cc, st, tm = _prompt(2007)
            twin.restart(1, cc, ac, st, tm, noise_seed=4107)
        Y.append(twin.step(X[:, k * 2048:(k + 1) * 2048]))
    codes1 = twin.pred_codes(1)
    twin.close()
    Y = np.concatenate(Y, axis=1)
    Y[1, :k0 * 2048] = 0.0
    y1 = E.test_resample(Y, MODEL, 48000)[1]
    L = run["L"]
    want = np.concatenate([run48["out"][1, :L + r0], y1[r0:]])[:N48]
    assert want.shape[0] == N48
    np.testing.assert_array_equal(_bits(run["out"][1]), _bits(want))
    np.testing.assert_array_equal(run["codes"][1], codes1)


def test_process_device_is_ordered_with_the_callers_stream(eng, run48):
    """sva_io_process_device on torch's current stream (the default one), pipelined, join_output = 1, no host synchronisation between the
    calls: the caller fills d_in and reads d_out with kernels of its own stream around every call, reusing both buffers.  Bit for bit what
    process() returns."""
    x = _source(2229 * 9)[:, :N48]
    b = _batch(eng, pipeline=True)
    io = b.open_io(48000, "f32", max_block=480)
    n_calls = N48 // 480
    X = torch.from_numpy(x.reshape(B, n_calls, 480).transpose(1, 0, 2).copy()).cuda()        # [calls][B][480]
    outs = torch.zeros(n_calls, B, 480, device="cuda")
    d_in, d_out = torch.empty(B, 480, device="cuda"), torch.empty(B, 480, device="cuda")
    torch.cuda.synchronize()
    for i in range(n_calls):
        d_in.copy_(X[i])                                   # a kernel on the caller's stream: the engine's read waits for it
        io.process_device(d_in.data_ptr(), d_out.data_ptr(), 480)
        outs[i].copy_(d_out)                               # ... and this one waits for the engine's pop
        d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    b.sync()
    got = outs.cpu().numpy().transpose(1, 0, 2).reshape(B, N48)
    codes = [b.pred_codes(s) for s in range(B)]
    b.close()
    np.testing.assert_array_equal(_bits(got), _bits(run48["out"]))
    for s in range(B):
        np.testing.assert_array_equal(codes[s], run48["codes"][s])


def test_refusals_change_nothing(eng, run48):
    run = _adaptor_run(eng, _source(2229 * 9)[:, :N48], 48000, 480, events={0: [("refusals",)], 20: [("refusals",)]})
    np.testing.assert_array_equal(_bits(run["out"]), _bits(run48["out"]))
    for s in range(B):
        np.testing.assert_array_equal(run["codes"][s], run48["codes"][s])
    from streamvoiceanon_amd import engine as E

    b = _batch(eng)
    with pytest.raises(RuntimeError, match="reduced by their gcd"):
        b.open_io(47999)
    assert b.io is None
    io = b.open_io(16000, "i16", 320)
    with pytest.raises(RuntimeError, match="one per batch"):
        E.BatchIO(b, 48000)
    assert io.process(np.zeros((B, 320), np.int16)).dtype == np.int16
    b.close()                                              # (closes the adaptor it still has)


def test_server_ioconf_16k_int16(weights0):
    """IOCONF to 16 kHz int16: 320-sample blocks come back as 320-sample int16 blocks, equal to BatchIO.process of the same samples"""
    import threading

    from streamvoiceanon_amd import stream_server as S
    from streamvoiceanon_amd.infer_arvc import InferenceWrapper
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

    _, _, style, timbre = synth_prompt(2500, 8)
    ref = synth_utterance(7300, 2048 * 70 + 100)
    src = np.clip(np.rint(synth_utterance(7302, 320 * 30) * 32768.0), -32768, 32767).astype(np.int16)

    def make():
        w = InferenceWrapper(weights=weights0)
        w.style_encoder = lambda wav: style
        w.timbre_encoder = lambda wav: timbre
        return w

    w_srv, w_ref = make(), make()
    ready = threading.Event()
    th = threading.Thread(target=S.serve, args=(w_srv, "127.0.0.1", 0, 1, ready), daemon=True)
    th.start()
    assert ready.wait(30)
    c = S.Client(port=ready.port)
    c.configure(alpha=1.0, block_frame=1, n_frame_delay=2)
    c.set_reference("a.wav", ref)
    c.configure_io(16000, 1, 320)
    w_ref.prefill_prompt(ref, max_prompt_frames=64, delay=2, alpha=1.0)
    w_ref.setup_stream_caches(encode_window_frames=64, decode_window_frames=64, max_seq_frames=768, buffer_frames=32, decode_chunk_frames=1,
                              io_rate=16000, io_fmt="i16", io_max_block=320)
    got = []
    for i in range(30):
        blk = src[320 * i:320 * (i + 1)]
        got.append(c.convert(blk))
        assert got[-1].dtype == np.int16 and got[-1].shape == (320,)
        np.testing.assert_array_equal(got[-1], w_ref.batch.io.process(blk[None])[0])
    assert np.abs(np.concatenate(got)).max() > 30
    with pytest.raises(RuntimeError, match="refused"):
        c.convert(np.zeros(321, np.int16))                 # the BLOCK bound follows max_block (the server drops the connection)
    c.sock.close()
    th.join(30)
    w_srv.close(); w_ref.close()
    w_srv.engine.close(); w_ref.engine.close()
