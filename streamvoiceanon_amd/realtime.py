"""Audio-callback entry of the real-time front-end: the per-block function the reference GUI calls from
its sounddevice callback, `custom_infer` (evaluations/real-time-gui.py:32-49), over this package's InferenceWrapper.

Same contract: the prompt is (re)computed and the stream caches are rebuilt lazily, only when the reference name or the block
size (in 2048-sample frames) changed since the previous call (:36-47, GUI settings: max_prompt_frames = 64, encode window 64,
decode window 64, max_seq_frames 768, buffer_frames 32); every call then converts one block with `process_one_chunk` (:48).
The reference keeps that state in module globals (:27-28); `RealtimeSession` holds it per instance, and the module-level
`custom_infer` keeps one default session so the reference's call sites work unchanged.

The GUI's quick presets (:629-662, file configs/presets.json: name -> {description, alpha, block_frame, n_frame_delay}) set the
three arguments this entry takes from the GUI -- alpha (noise mixing of the speaker embeddings), block_frame (frames per audio
block = decode_chunk_frames) and n_frame_delay -- so they are part of this boundary: `load_presets` / `apply_preset` /
`RealtimeSession.run_block`.

The GUI itself (customtkinter / sounddevice, :61-1461) is a caller of this boundary and is not part of the engine.
"""
import dataclasses
import json
import struct

import numpy as np


@dataclasses.dataclass
class GuiSettings:
    """The three `gui_config` fields a preset writes (real-time-gui.py:645-660) with the GUI's start-up values."""
    alpha: float = 0.7
    block_frame: int = 1
    n_frame_delay: int = 2


def load_presets(path="configs/presets.json"):
    """real-time-gui.py:634-640: the JSON object of the file, {} if it cannot be read."""
    try:
        with open(path, "r") as f:
            return json.load(f)
    except Exception:
        return {}


def apply_preset(settings: GuiSettings, name: str, presets: dict) -> GuiSettings:
    """real-time-gui.py:641-662: "Custom" or an unknown name changes nothing; otherwise each of the three keys present in the preset
    overwrites the setting (block_frame / n_frame_delay as ints)."""
    if name == "Custom" or name not in presets:
        return settings
    p = presets[name]
    out = dataclasses.replace(settings)
    if "alpha" in p:
        out.alpha = float(p["alpha"])
    if "block_frame" in p:
        out.block_frame = int(p["block_frame"])
    if "n_frame_delay" in p:
        out.n_frame_delay = int(p["n_frame_delay"])
    return out


# the stream parameters of the GUI (real-time-gui.py:36-47), in ONE place: custom_infer sets its caches up with them and a loaded snapshot must
# have been taken under them (a second copy that drifted would turn every load into a configuration refusal)
MAX_PROMPT_FRAMES = 64
STREAM_CACHES = dict(encode_window_frames=64, decode_window_frames=64, max_seq_frames=768, buffer_frames=32)


class RealtimeSession:
    def __init__(self):
        self.reference_wav_name = ""
        self.decode_chunk_frames = 0
        self.prefills = 0                    # how many times the prompt was rebuilt (tests, diagnostics)
        self.io = None                       # (samplerate, format, max block) of the open I/O adaptor

    def custom_infer(self, model_set, reference_wav, new_reference_wav_name, input_wav, n_frame_delay=2, alpha=0.7, samplerate=44100,
                     block_frame=1, max_block=None):
        """reference_wav: float array at 44.1 kHz; input_wav: [2048 * k] block (torch tensor or array) -> converted block of the
        same kind and length (zeros while the decoder delay fills, infer_arvc.py:519-525).

        samplerate != 44100 is the GUI's sr_device mode (real-time-gui.py:1222-1230, 1340-1341: the sound device's own rate): input_wav is
        a block of ANY length at that rate, float32 or int16, and the converted block comes back at that rate, length and format, resampled
        on the device (engine.BatchIO) and delayed by model_set.batch.io.latency samples.  block_frame = decode chunk frames of the engine
        underneath; max_block = the longest block that will come (default: twice this one, at least 4096).  With max_block given the adaptor
        is used at 44100 too: its pass-through takes any block length and int16 there."""
        if int(samplerate) != 44100 or max_block is not None:      # (max_block: the caller asks for the adaptor, also for its 44.1 kHz pass-through)
            return self._infer_at_rate(model_set, reference_wav, new_reference_wav_name, input_wav, n_frame_delay, alpha, int(samplerate),
                                       int(block_frame), max_block)
        n = int(input_wav.shape[-1])
        assert n % 2048 == 0 and n > 0, "block size must be a whole number of 2048-sample frames"
        frames = n // 2048
        if self.reference_wav_name != new_reference_wav_name or self.decode_chunk_frames != frames or self.io is not None:
            ref = np.asarray(reference_wav.detach().cpu().numpy() if hasattr(reference_wav, "detach") else reference_wav, dtype=np.float32)
            model_set.prefill_prompt(ref.reshape(-1), max_prompt_frames=MAX_PROMPT_FRAMES, delay=n_frame_delay, alpha=alpha)
            model_set.setup_stream_caches(decode_chunk_frames=frames, **STREAM_CACHES)
            self.reference_wav_name = new_reference_wav_name
            self.decode_chunk_frames = frames
            self.io = None
            self.prefills += 1
        is_torch = hasattr(input_wav, "detach")
        block = input_wav.reshape(1, -1) if not is_torch else input_wav.reshape(1, -1)
        pred = model_set.process_one_chunk(block)
        return pred.squeeze() if is_torch else np.asarray(pred).reshape(-1)

    def _infer_at_rate(self, model_set, reference_wav, new_reference_wav_name, input_wav, n_frame_delay, alpha, samplerate, block_frame, max_block):
        is_torch = hasattr(input_wav, "detach")
        x = input_wav.detach().cpu().numpy() if is_torch else np.asarray(input_wav)
        fmt = "i16" if x.dtype == np.int16 else "f32"
        n = int(x.shape[-1])
        assert n > 0, "empty block"
        io = self.io
        if (self.reference_wav_name != new_reference_wav_name or self.decode_chunk_frames != block_frame or io is None or io[:2] != (samplerate, fmt)
                or n > io[2]):
            ref = np.asarray(reference_wav.detach().cpu().numpy() if hasattr(reference_wav, "detach") else reference_wav, dtype=np.float32)
            cap = int(max_block) if max_block else max(4096, 2 * n)
            assert n <= cap, "block longer than max_block"
            model_set.prefill_prompt(ref.reshape(-1), max_prompt_frames=MAX_PROMPT_FRAMES, delay=n_frame_delay, alpha=alpha)
            model_set.setup_stream_caches(decode_chunk_frames=block_frame, io_rate=samplerate, io_fmt=fmt, io_max_block=cap, **STREAM_CACHES)
            self.reference_wav_name = new_reference_wav_name
            self.decode_chunk_frames = block_frame
            self.io = (samplerate, fmt, cap)
            self.prefills += 1
        pred = np.asarray(model_set.process_one_chunk(x.reshape(1, -1))).reshape(-1)
        if is_torch:
            import torch

            return torch.from_numpy(pred).to(input_wav.device)
        return pred


    # ---- save / resume: the engine's snapshot of the session's stream in a small envelope ----
    # b"SVARTS1\0" | u32 name bytes | u32 chunk frames | u32 n_frame_delay | utf-8 reference name | engine blob   (little endian)
    ENVELOPE_MAGIC = b"SVARTS1\0"

    def save(self, model_set) -> bytes:
        """The session's live stream (engine.Batch.save_stream) with what custom_infer keys its lazy re-prefill on.  Needs a stream whose
        delay has filled; refused while an I/O adaptor is open (its FIFOs are batch-wide and do not travel)."""
        if self.io is not None:
            raise RuntimeError("save refused: an I/O adaptor is open on this session; its FIFOs and phase counters are batch-wide and do not travel")
        if not self.reference_wav_name or not self.decode_chunk_frames:
            raise RuntimeError("save refused: the session has no stream yet (send a reference and a block first)")
        name = self.reference_wav_name.encode("utf-8")
        return self.ENVELOPE_MAGIC + struct.pack("<III", len(name), self.decode_chunk_frames, int(model_set.delay)) + name + model_set.save_stream()

    def load(self, model_set, data):
        """Continue the stream of a save() envelope: the next custom_infer with that reference name (and block size) does NOT re-prefill
        (`prefills` unchanged) -- the reference is neither encoded nor prefilled again."""
        if self.io is not None:
            raise RuntimeError("load refused: an I/O adaptor is open on this session; its FIFOs and phase counters are batch-wide and do not travel")
        data = bytes(data)
        m = len(self.ENVELOPE_MAGIC)
        if len(data) < m + 12 or data[:m] != self.ENVELOPE_MAGIC:
            raise ValueError("not a session envelope (RealtimeSession.save)")
        n_name, frames, delay = struct.unpack("<III", data[m:m + 12])
        if n_name > 1024 or len(data) < m + 12 + n_name or not 1 <= frames <= 64 or delay < 1:
            raise ValueError("session envelope: bad name length, chunk frames or delay")
        name = data[m + 12:m + 12 + n_name].decode("utf-8")
        # A refused blob leaves the session as it was when the wrapper kept its live batch.  When the wrapper had to replace the batch by a
        # landing batch first, the session forgets its stream: the next block then re-prefills from its reference instead of stepping a
        # retired slot.
        keep, before = (self.reference_wav_name, self.decode_chunk_frames), getattr(model_set, "batch", None)
        self.reference_wav_name, self.decode_chunk_frames = "", 0
        try:
            model_set.load_stream(data[m + 12 + n_name:], decode_chunk_frames=int(frames), delay=int(delay), max_prompt_frames=MAX_PROMPT_FRAMES,
                                  **STREAM_CACHES)
        except Exception:
            if before is not None and getattr(model_set, "batch", None) is before:
                self.reference_wav_name, self.decode_chunk_frames = keep
            raise
        self.reference_wav_name = name
        self.decode_chunk_frames = int(frames)
        return name, int(frames), int(delay)

    def run_block(self, model_set, reference_wav, reference_wav_name, input_wav, settings: GuiSettings):
        """One audio-callback block under the GUI's current settings (real-time-gui.py:1313-1330 passes gui_config.n_frame_delay and
        gui_config.alpha; block_frame fixes the block length the callback delivers)."""
        assert int(input_wav.shape[-1]) == 2048 * settings.block_frame, "the audio callback delivers block_frame frames per block"
        return self.custom_infer(model_set, reference_wav, reference_wav_name, input_wav, n_frame_delay=settings.n_frame_delay,
                                 alpha=settings.alpha)


_default = RealtimeSession()


def custom_infer(model_set, reference_wav, new_reference_wav_name, input_wav, n_frame_delay=2, alpha=0.7, samplerate=44100, block_frame=1,
                 max_block=None):
    """real-time-gui.py:32-49 with the module-global state of the reference (one default session)."""
    return _default.custom_infer(model_set, reference_wav, new_reference_wav_name, input_wav, n_frame_delay=n_frame_delay, alpha=alpha,
                                 samplerate=samplerate, block_frame=block_frame, max_block=max_block)
