"""Host side of save / resume without a GPU: RealtimeSession's envelope and the server's SAVE / LOAD frames against a stub model set."""
import struct
import threading

import numpy as np
import pytest


class Stub:
    """what RealtimeSession and the server need of an InferenceWrapper"""

    def __init__(self):
        self.prefills, self.loads, self.delay = 0, [], 0
        self.batch = object()                  # the live batch: a refused load that leaves it in place leaves the session alone too

    def prefill_prompt(self, ref, max_prompt_frames=64, delay=2, alpha=1.0):
        self.prefills += 1
        self.delay = delay

    def setup_stream_caches(self, **kw):
        pass

    def process_one_chunk(self, block):
        return np.asarray(block) * 0.5

    def save_stream(self):
        return b"ENGINE-BLOB" * 3

    def load_stream(self, blob, **kw):
        if not blob.startswith(b"ENGINE-BLOB"):
            raise RuntimeError("sva_stream_load failed (rc=-11): not a stream snapshot (wrong magic)")
        self.loads.append((bytes(blob), kw))


def test_session_envelope_round_trip():
    from streamvoiceanon_amd.realtime import RealtimeSession

    m, s = Stub(), RealtimeSession()
    with pytest.raises(RuntimeError, match="no stream yet"):
        s.save(m)
    x = np.ones(2 * 2048, np.float32)
    s.custom_infer(m, np.ones(2048 * 4, np.float32), "réf.wav", x, n_frame_delay=3, alpha=1.0)
    env = s.save(m)
    name = "réf.wav".encode("utf-8")
    assert env == b"SVARTS1\0" + struct.pack("<III", len(name), 2, 3) + name + b"ENGINE-BLOB" * 3
    m2, s2 = Stub(), RealtimeSession()
    assert s2.load(m2, env) == ("réf.wav", 2, 3)
    assert m2.loads == [(b"ENGINE-BLOB" * 3, dict(encode_window_frames=64, decode_window_frames=64, max_seq_frames=768, buffer_frames=32,
                                                  decode_chunk_frames=2, delay=3, max_prompt_frames=64))]
    s2.custom_infer(m2, None, "réf.wav", x, n_frame_delay=3, alpha=1.0)          # same name, same block size: no re-prefill, the reference is not touched
    assert s2.prefills == 0 and m2.prefills == 0
    s2.custom_infer(m2, np.ones(2048 * 4, np.float32), "other.wav", x, n_frame_delay=3, alpha=1.0)
    assert s2.prefills == 1
    for bad in (b"", env[:12], b"X" + env[1:], env[:8] + struct.pack("<III", 5000, 2, 3) + env[20:], env[:8] + struct.pack("<III", len(name), 0, 3) + env[20:]):
        with pytest.raises(ValueError, match="envelope"):
            RealtimeSession().load(Stub(), bad)
    with pytest.raises(RuntimeError, match="wrong magic"):                        # the engine's refusal passes through, the session keeps its state
        s2.load(m2, env[:20 + len(name)] + b"garbage")
    assert s2.reference_wav_name == "other.wav" and s2.decode_chunk_frames == 2
    m2.batch = None                                                               # ... but a wrapper that lost its live batch on the way: the session forgets its stream
    with pytest.raises(RuntimeError, match="wrong magic"):
        s2.load(m2, env[:20 + len(name)] + b"garbage")
    assert s2.reference_wav_name == "" and s2.decode_chunk_frames == 0
    s2.custom_infer(m2, np.ones(2048 * 4, np.float32), "other.wav", x, n_frame_delay=3, alpha=1.0)
    assert s2.prefills == 2                                                       # the next block re-prefills instead of stepping an empty slot
    s2.io = (48000, "f32", 4096)
    with pytest.raises(RuntimeError, match="I/O adaptor"):
        s2.save(m2)
    with pytest.raises(RuntimeError, match="I/O adaptor"):
        s2.load(m2, env)


def test_server_save_and_load_frames_with_a_stub_model():
    from streamvoiceanon_amd import stream_server as S

    stub, ready = Stub(), threading.Event()
    th = threading.Thread(target=S.serve, args=(stub, "127.0.0.1", 0, 3, ready), daemon=True)
    th.start()
    assert ready.wait(10)
    x = np.arange(2048, dtype=np.float32)
    c = S.Client(port=ready.port)
    with pytest.raises(RuntimeError, match="no stream yet"):
        c.save()
    c.set_reference("r1", np.ones(2048 * 4, np.float32))
    c.configure(alpha=1.0, block_frame=1, n_frame_delay=2)
    c.convert(x)
    env = c.save()
    assert env.startswith(b"SVARTS1\0") and env.endswith(b"ENGINE-BLOB")
    c.close()
    c = S.Client(port=ready.port)
    with pytest.raises(RuntimeError, match="reference"):
        c.convert(x)                                           # a fresh session still needs a REF or a LOAD
    with pytest.raises(RuntimeError, match="envelope"):
        c.load(b"nonsense")
    c.load(env)
    np.testing.assert_array_equal(c.convert(x), x * 0.5)       # no REF on this connection
    assert stub.prefills == 1 and len(stub.loads) == 1
    c.configure_io(sample_rate=48000, fmt=0, max_block=4096)
    with pytest.raises(RuntimeError, match="IOCONF"):
        c.save()
    with pytest.raises(RuntimeError, match="IOCONF"):
        c.load(env)
    c.close()
    # a LOAD frame beyond the engine's largest possible snapshot is refused before its payload is read, and the connection is dropped
    assert S.max_load_bytes(stub) == 12 * 2 * 12 * 64 * 4 * 2048 + (16 << 20) + 2048
    c = S.Client(port=ready.port)
    S._send(c.sock, S.KIND_SAVE, b"x")                          # SAVE carries no payload
    k, n = struct.unpack("<II", S._recv_exact(c.sock, 8))
    assert k == S.KIND_ERR and b"refused" in S._recv_exact(c.sock, n)
    try:
        assert c.sock.recv(1) == b""
    except ConnectionResetError:                                # (the unread payload byte turns the server's close into a reset)
        pass
    c.sock.close()
    th.join(10)
    assert not th.is_alive()
