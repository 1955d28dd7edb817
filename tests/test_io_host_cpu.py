"""Host side of the I/O adaptor without a GPU: RealtimeSession.custom_infer(samplerate=) and the server's IOCONF frame against a stub model
set -- what reaches setup_stream_caches, when the caches are rebuilt, which block lengths and formats are accepted, and that the default
44.1 kHz path asks for nothing new."""
import threading

import numpy as np
import pytest


class Stub:
    def __init__(self):
        self.prefills, self.setups = 0, []

    def prefill_prompt(self, ref, max_prompt_frames=64, delay=2, alpha=1.0):
        self.prefills += 1

    def setup_stream_caches(self, **kw):
        self.setups.append(kw)

    def process_one_chunk(self, block):
        b = np.asarray(block)
        return (b // 2).astype(b.dtype) if b.dtype == np.int16 else b * 0.5


REF = np.ones(2048 * 4, np.float32)


def test_custom_infer_at_a_device_rate():
    from streamvoiceanon_amd.realtime import RealtimeSession

    stub, sess = Stub(), RealtimeSession()
    x = np.arange(960, dtype=np.float32)
    out = sess.custom_infer(stub, REF, "r", x[:480], samplerate=48000)
    assert out.shape == (480,) and out.dtype == np.float32
    np.testing.assert_array_equal(out, x[:480] * 0.5)
    assert stub.setups[-1]["io_rate"] == 48000 and stub.setups[-1]["io_fmt"] == "f32" and stub.setups[-1]["io_max_block"] >= 4096
    assert stub.setups[-1]["decode_chunk_frames"] == 1
    sess.custom_infer(stub, REF, "r", x[:37], samplerate=48000)              # another block length: same caches
    sess.custom_infer(stub, REF, "r", x, samplerate=48000)
    assert sess.prefills == 1 and len(stub.setups) == 1
    xi = np.arange(320, dtype=np.int16)
    oi = sess.custom_infer(stub, REF, "r", xi, samplerate=16000, block_frame=2, max_block=320)
    assert oi.dtype == np.int16 and oi.shape == (320,)
    assert (stub.setups[-1]["io_rate"], stub.setups[-1]["io_fmt"], stub.setups[-1]["io_max_block"], stub.setups[-1]["decode_chunk_frames"]) == (16000, "i16", 320, 2)
    assert sess.prefills == 2
    with pytest.raises(AssertionError, match="max_block"):
        sess.custom_infer(stub, REF, "r", np.zeros(321, np.int16), samplerate=16000, block_frame=2, max_block=320)
    # back to the default: whole chunks of float32 at 44.1 kHz, caches rebuilt without an adaptor, the 2048 rule as before
    out = sess.custom_infer(stub, REF, "r", np.zeros(2048, np.float32))
    assert out.shape == (2048,) and "io_rate" not in stub.setups[-1]
    with pytest.raises(AssertionError, match="2048"):
        sess.custom_infer(stub, REF, "r", np.zeros(480, np.float32))


def test_default_path_passes_no_adaptor_arguments():
    from streamvoiceanon_amd.realtime import RealtimeSession

    stub, sess = Stub(), RealtimeSession()
    sess.custom_infer(stub, REF, "r", np.zeros(4096, np.float32))
    sess.custom_infer(stub, REF, "r", np.zeros(4096, np.float32))
    assert sess.prefills == 1 and len(stub.setups) == 1
    assert sorted(stub.setups[0]) == ["buffer_frames", "decode_chunk_frames", "decode_window_frames", "encode_window_frames", "max_seq_frames"]


def test_server_ioconf_frame():
    from streamvoiceanon_amd import stream_server as S

    stub, ready = Stub(), threading.Event()
    th = threading.Thread(target=S.serve, args=(stub, "127.0.0.1", 0, 1, ready), daemon=True)
    th.start()
    assert ready.wait(10)
    c = S.Client(port=ready.port)
    c.set_reference("r", REF)
    c.configure(alpha=0.5, block_frame=1, n_frame_delay=3)
    with pytest.raises(RuntimeError, match="fmt"):
        c.configure_io(16000, 7, 320)
    with pytest.raises(RuntimeError):
        S.Client._roundtrip(c, S.KIND_IOCONF, b"\0" * 5)             # short payload: an error frame, the connection survives
    with pytest.raises(RuntimeError, match="reduced by their gcd"):
        c.configure_io(47999, 0, 480)                                         # the rate rule is checked here, not at the first block
    assert stub.prefills == 0
    c.configure_io(44100, 1, 1000)                                            # int16 at 44.1 kHz: the adaptor's pass-through, any length
    np.testing.assert_array_equal(c.convert(np.arange(500, dtype=np.int16)), np.arange(500, dtype=np.int16) // 2)
    assert (stub.setups[-1]["io_rate"], stub.setups[-1]["io_fmt"], stub.setups[-1]["io_max_block"]) == (44100, "i16", 1000)
    c.configure_io(16000, 1, 320)
    x = np.arange(-160, 160, dtype=np.int16)
    got = c.convert(x)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, x // 2)
    np.testing.assert_array_equal(c.convert(x[:100]), x[:100] // 2)           # any length up to max_block, no rebuild
    assert stub.prefills == 2 and (stub.setups[-1]["io_rate"], stub.setups[-1]["io_fmt"], stub.setups[-1]["io_max_block"]) == (16000, "i16", 320)
    c.configure_io(44100, 0, 4096)                                            # back to whole float32 chunks
    np.testing.assert_array_equal(c.convert(np.ones(2048, np.float32)), np.full(2048, 0.5, np.float32))
    with pytest.raises(RuntimeError, match="block_frame"):
        c.convert(np.ones(480, np.float32))
    c.configure_io(8000, 1, 160)
    with pytest.raises(RuntimeError, match="refused"):
        c.convert(np.zeros(161, np.int16))                                    # the BLOCK bound follows max_block: refused unread, connection dropped
    c.sock.close()
    th.join(10)
    assert not th.is_alive()
