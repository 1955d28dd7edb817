"""A small streaming server over the real-time boundary.

The reference's live front-end is a customtkinter GUI whose sounddevice callback (evaluations/real-time-gui.py:1204-1358) feeds
`custom_infer` one audio block at a time, re-prefilling lazily when the reference or the block size changes (:32-49).  The GUI toolkit
and the sound device are callers of that loop, not part of the engine; this module is the same loop behind a socket, so that any
client (a sound-card bridge, a VoIP hop, a test) can stream blocks through one GPU-resident session:

    python -m streamvoiceanon_amd.stream_server --port 5577 [--config_path ... --checkpoint_path ...]

Protocol (little endian, one TCP connection = one `RealtimeSession`):
    client -> server   frame  = u32 kind | u32 nbytes | payload
        kind 1 REF    payload = utf-8 name, 0 byte, float32 samples at 44.1 kHz     (a new reference: next block re-prefills, :36-47)
        kind 2 CONF   payload = float32 alpha | i32 block_frame | i32 n_frame_delay (the three GUI settings a preset writes, :645-660)
        kind 3 BLOCK  payload = float32[2048 * block_frame] source samples
        kind 4 BYE
        kind 5 IOCONF payload = i32 sample_rate | i32 fmt (0 float32, 1 int16) | i32 max_block: from here on a BLOCK is max_block or fewer
                      samples of that format at that rate (any length: a 10 ms sound-card or telephony callback) and is answered with as
                      many samples of that format at that rate, resampled on the device (engine.BatchIO; the GUI's sr_device mode);
                      sample_rate 44100 with fmt 0 goes back to whole-chunk float32 blocks (44100 with fmt 1 is the adaptor's pass-through).  block_frame of CONF stays the engine's chunk.
        kind 6 SAVE   no payload: the session's live stream is answered as an envelope (RealtimeSession.save: reference name, chunk frames,
                      delay, then the engine's snapshot -- include/sva.h, sva_stream_save); the stream goes on
        kind 7 LOAD   payload = such an envelope: the session continues that stream; the BLOCKs that follow need no REF and do not re-prefill
                      (the envelope's reference name and chunk frames become the session's; a later REF with another name starts afresh)
                      SAVE and LOAD are refused after an IOCONF: the adaptor's FIFOs and phase counters are batch-wide and do not travel
    server -> client   for every BLOCK: u32 3 | u32 nbytes | float32[2048 * block_frame] converted samples (zeros while the delay fills)
                       for REF / CONF / IOCONF / LOAD:  u32 kind | u32 0;   for SAVE:  u32 6 | u32 nbytes | envelope
                       on error:        u32 0xffffffff | u32 nbytes | utf-8 message (the connection stays open)
    Frame sizes are bounded per kind (CONF = IOCONF = 12 bytes, BLOCK <= 64 frames of 2048 samples -- after an IOCONF: max_block samples --, REF <= 60 s of 44.1 kHz audio + a 1 KiB name,
    LOAD <= the engine's largest possible snapshot -- every KV position of the cache -- + 16 MiB for everything else + the envelope);
    an oversize or unknown frame is answered with an error and the connection is closed (its payload cannot be skipped safely).

One connection is served at a time per process (the reference's GUI is single-session too); the engine and its weights stay
resident between connections.
"""
import argparse
import socket
import struct

import numpy as np

from .engine import io_rate_supported
from .realtime import GuiSettings, RealtimeSession

KIND_REF, KIND_CONF, KIND_BLOCK, KIND_BYE, KIND_IOCONF, KIND_SAVE, KIND_LOAD, KIND_ERR = 1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF
MAX_BLOCK_FRAMES = 64
MAX_PAYLOAD = {KIND_REF: 1024 + 1 + 4 * 44100 * 60, KIND_CONF: 12, KIND_BLOCK: 4 * 2048 * MAX_BLOCK_FRAMES, KIND_BYE: 0, KIND_IOCONF: 12}
IO_DTYPES = {0: "<f4", 1: "<i2"}


IO_REFUSAL = "refused after an IOCONF: the I/O adaptor's FIFOs and phase counters are batch-wide and do not travel with a stream"


def max_load_bytes(model_set):
    """Size bound of a LOAD frame: the engine's largest possible snapshot (KV rows up to the end of the cache dominate; everything else together is
    a few MB) plus the envelope.  A model set without an engine (a stub) gets the bound of the default configuration."""
    cfg = getattr(getattr(model_set, "engine", None), "cfg", None)
    layers, heads, seq, half = (cfg.ar_layers, cfg.ar_heads, cfg.max_seq_len, cfg.ar_dtype == 1) if cfg is not None else (12, 12, 2048, False)
    return layers * 2 * heads * 64 * (2 if half else 4) * seq + (16 << 20) + 2048


class ProtocolError(Exception):
    """A frame the server cannot even read past (unknown kind, oversize payload): answered, then the connection is dropped."""


def _recv_exact(conn, n):
    buf = bytearray()
    while len(buf) < n:
        chunk = conn.recv(n - len(buf))
        if not chunk:
            raise ConnectionError("peer closed the connection")
        buf += chunk
    return bytes(buf)


def _send(conn, kind, payload=b""):
    conn.sendall(struct.pack("<II", kind, len(payload)) + payload)


def serve_connection(conn, model_set):
    """The audio loop of real-time-gui.py:1313-1330 for one client: every BLOCK goes through RealtimeSession.run_block."""
    sess, settings = RealtimeSession(), GuiSettings()
    ref_name, ref_wav = "", None
    loaded = False                           # a LOAD gave the session its stream: BLOCKs need no REF until one arrives
    ioconf = None                            # (sample_rate, fmt, max_block) of the last IOCONF, None: 44.1 kHz float32 in whole chunks
    while True:
        kind, nbytes = struct.unpack("<II", _recv_exact(conn, 8))
        limits = {**MAX_PAYLOAD, KIND_SAVE: 0, KIND_LOAD: max_load_bytes(model_set)}
        if ioconf is not None:
            limits[KIND_BLOCK] = ioconf[2] * np.dtype(IO_DTYPES[ioconf[1]]).itemsize
        if kind not in limits or nbytes > limits[kind]:
            msg = f"frame kind {kind} with {nbytes} bytes refused (limits: {limits})"
            _send(conn, KIND_ERR, ("ProtocolError: " + msg).encode("utf-8"))
            raise ProtocolError(msg)
        payload = _recv_exact(conn, nbytes) if nbytes else b""
        try:
            if kind == KIND_BYE:
                return
            if kind == KIND_REF:
                z = payload.index(b"\0")
                ref_name = payload[:z].decode("utf-8")
                ref_wav = np.frombuffer(payload[z + 1:], dtype="<f4").astype(np.float32)
                loaded = False
                if ref_wav.size < 2048 * 3:
                    raise ValueError("reference shorter than three frames")
                _send(conn, KIND_REF)
            elif kind == KIND_CONF:
                alpha, bf, nd = struct.unpack("<fii", payload)
                if not (1 <= bf <= MAX_BLOCK_FRAMES and nd >= 1):
                    raise ValueError(f"block_frame must be 1..{MAX_BLOCK_FRAMES} and n_frame_delay >= 1")
                settings = GuiSettings(alpha=float(alpha), block_frame=int(bf), n_frame_delay=int(nd))
                _send(conn, KIND_CONF)
            elif kind == KIND_IOCONF:
                rate, fmt, max_block = struct.unpack("<iii", payload)
                if fmt not in IO_DTYPES or not 1 <= max_block <= 2048 * MAX_BLOCK_FRAMES:
                    raise ValueError(f"fmt must be 0 (float32) or 1 (int16) and max_block 1..{2048 * MAX_BLOCK_FRAMES}")
                if not io_rate_supported(rate):
                    raise ValueError(f"sample_rate {rate} refused: an integer in 8000 .. 96000 whose ratio to 44100, reduced by their gcd, "
                                     "has both terms <= 640")
                ioconf = None if (rate, fmt) == (44100, 0) else (int(rate), int(fmt), int(max_block))
                _send(conn, KIND_IOCONF)
            elif kind == KIND_SAVE:
                if ioconf is not None or sess.io is not None:
                    raise ValueError("SAVE " + IO_REFUSAL)
                _send(conn, KIND_SAVE, sess.save(model_set))
            elif kind == KIND_LOAD:
                if ioconf is not None or sess.io is not None:
                    raise ValueError("LOAD " + IO_REFUSAL)
                ref_name = sess.load(model_set, payload)[0]
                loaded = True
                _send(conn, KIND_LOAD)
            elif kind == KIND_BLOCK and ioconf is not None:
                if ref_wav is None:
                    raise ValueError("send a reference (kind 1) before the first block")
                dt = np.dtype(IO_DTYPES[ioconf[1]])
                if len(payload) % dt.itemsize or not payload:
                    raise ValueError("block payload is not a whole, positive number of samples")
                block = np.frombuffer(payload, dtype=dt).astype(dt.newbyteorder("="))
                out = sess.custom_infer(model_set, ref_wav, ref_name, block, n_frame_delay=settings.n_frame_delay, alpha=settings.alpha,
                                        samplerate=ioconf[0], block_frame=settings.block_frame, max_block=ioconf[2])
                _send(conn, KIND_BLOCK, np.ascontiguousarray(out, dtype=dt).tobytes())
            elif kind == KIND_BLOCK:
                if ref_wav is None and not loaded:
                    raise ValueError("send a reference (kind 1) before the first block")
                if len(payload) % 4:
                    raise ValueError("block payload is not a whole number of float32 samples")
                block = np.frombuffer(payload, dtype="<f4").astype(np.float32)
                out = sess.run_block(model_set, ref_wav, ref_name, block, settings)
                _send(conn, KIND_BLOCK, np.ascontiguousarray(out, dtype="<f4").tobytes())
        except (ValueError, AssertionError, RuntimeError, NotImplementedError, struct.error, UnicodeDecodeError) as ex:
            _send(conn, KIND_ERR, f"{type(ex).__name__}: {ex}".encode("utf-8"))


def serve(model_set, host="127.0.0.1", port=5577, max_connections=None, ready=None):
    """Accept connections one after the other.  `ready` (threading.Event-like) is set once the socket listens; the bound port is
    returned through `ready.port` when port = 0."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as srv:
        srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        srv.bind((host, port))
        srv.listen(1)
        if ready is not None:
            ready.port = srv.getsockname()[1]
            ready.set()
        served = 0
        while max_connections is None or served < max_connections:
            conn, _ = srv.accept()
            with conn:
                conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                try:
                    serve_connection(conn, model_set)
                except (ConnectionError, ProtocolError):
                    pass
                except Exception as ex:          # a misbehaving client must not take the resident engine down with it
                    print(f"stream_server: connection dropped after {type(ex).__name__}: {ex}", flush=True)
            served += 1


class Client:
    """Minimal client of the protocol (tests, bridges)."""

    def __init__(self, host="127.0.0.1", port=5577):
        self.sock = socket.create_connection((host, port))
        self.sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)

    def _roundtrip(self, kind, payload):
        _send(self.sock, kind, payload)
        k, n = struct.unpack("<II", _recv_exact(self.sock, 8))
        body = _recv_exact(self.sock, n) if n else b""
        if k == KIND_ERR:
            raise RuntimeError(body.decode("utf-8"))
        return body

    def set_reference(self, name, wav):
        self._roundtrip(KIND_REF, name.encode("utf-8") + b"\0" + np.ascontiguousarray(wav, dtype="<f4").tobytes())

    def configure(self, alpha=0.7, block_frame=1, n_frame_delay=2):
        self._roundtrip(KIND_CONF, struct.pack("<fii", alpha, block_frame, n_frame_delay))

    def configure_io(self, sample_rate=44100, fmt=0, max_block=4096):
        """IOCONF: blocks of any length up to max_block at sample_rate, float32 (fmt 0) or int16 (fmt 1)"""
        self._roundtrip(KIND_IOCONF, struct.pack("<iii", sample_rate, fmt, max_block))
        self.dtype = IO_DTYPES[fmt]

    def save(self) -> bytes:
        """SAVE: the session's live stream as an envelope (RealtimeSession.save)"""
        return self._roundtrip(KIND_SAVE, b"")

    def load(self, envelope):
        """LOAD: continue the stream of a save() envelope; no set_reference is needed before the next convert"""
        self._roundtrip(KIND_LOAD, bytes(envelope))

    def convert(self, block):
        dt = getattr(self, "dtype", "<f4")
        return np.frombuffer(self._roundtrip(KIND_BLOCK, np.ascontiguousarray(block, dtype=dt).tobytes()), dtype=dt).copy()

    def close(self):
        try:
            _send(self.sock, KIND_BYE)
        finally:
            self.sock.close()


def main(argv=None):
    from .infer_arvc import InferenceWrapper

    ap = argparse.ArgumentParser(description="StreamVoiceAnon streaming server (MI355X engine)")
    ap.add_argument("--config_path", type=str, default="configs/config_firefly_arvcasr_8192_delay0_8.yaml")
    ap.add_argument("--checkpoint_path", type=str, default=None)
    ap.add_argument("--host", type=str, default="127.0.0.1")
    ap.add_argument("--port", type=int, default=5577)
    ap.add_argument("--fp16", action="store_true", help="fp16 AR weights + KV cache (the reference's InferenceWrapper(fp16=True))")
    ap.add_argument("--enc-fp16", action="store_true", help="content encoder GEMMs on fp16 operands, fp32 accumulate (sva_config.enc_dtype = 1)")
    args = ap.parse_args(argv)
    model_set = InferenceWrapper(args.config_path, args.checkpoint_path, fp16=args.fp16, enc_dtype=1 if args.enc_fp16 else 0)
    print(f"listening on {args.host}:{args.port}", flush=True)
    serve(model_set, args.host, args.port)


if __name__ == "__main__":
    main()
