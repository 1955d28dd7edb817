"""Host side of slot-local activation (sva_stream_params.slot_priming): the default, the exported counter call, and the continuous-batching
scheduler's independence of the flag.  No GPU, no compute calls."""
import ctypes
import inspect
import types

import numpy as np

N = 2048


def test_default_is_whole_batch_priming():
    from streamvoiceanon_amd import engine as E

    lib = E.load_library()
    p = E.SvaStreamParams()
    p.slot_priming = 7
    assert lib.sva_stream_params_default(ctypes.byref(p)) == 0
    assert p.slot_priming == 0
    assert E.SvaStreamParams._fields_[-1] == ("slot_priming", ctypes.c_int)          # appended: every earlier field keeps its offset
    assert inspect.signature(E.Batch.__init__).parameters["slot_priming"].default is False


def test_activation_counters_exported():
    from streamvoiceanon_amd import engine as E

    lib = ctypes.CDLL(E.LIB_PATH)
    assert hasattr(lib, "sva_stream_activations")
    assert "sva_stream_activations" in E.EXPORTED_SYMBOLS
    assert callable(E.Batch.activations)
    counts = (ctypes.c_long * 2)(5, 5)
    assert E.load_library().sva_stream_activations(None, counts, None) != 0           # refuses a null batch, writes nothing
    assert list(counts) == [5, 5] and b"null" in E.load_library().sva_last_error()


class _FakeBatch:
    """Records how it was created and what the scheduler asks of it; output = input + 1000 * (tag of the slot's prompt)."""
    made = []

    def __init__(self, engine, n_streams=1, **kw):
        self.kw, self.n, self.tag, self.calls = dict(kw, n_streams=n_streams), n_streams, [None] * n_streams, []
        self.idle = [False] * n_streams
        _FakeBatch.made.append(self)

    def prefill_prompt(self, slot, cc, ac, st, tm, noise_seed=0):
        self.tag[slot] = int(cc[0])

    def begin(self):
        self.calls.append(("begin",))

    def restart(self, slot, cc, ac, st, tm, noise_seed=0):
        self.calls.append(("restart", slot, int(cc[0]), int(noise_seed)))
        self.tag[slot], self.idle[slot] = int(cc[0]), False

    def retire(self, slot):
        self.calls.append(("retire", slot))
        self.idle[slot] = True

    def step(self, x):
        self.calls.append(("step",))
        out = np.zeros_like(x)
        for s in range(self.n):
            if not self.idle[s]:
                out[s] = x[s] + 1000.0 * self.tag[s]
        return out

    def close(self):
        pass


def test_scheduler_does_not_depend_on_the_flag(monkeypatch):
    """stream_infer_many hands slot_priming to its batch and to nothing else: run_pool / SlotPool have no such parameter and make the
    same calls, in the same order, with the same PCM routing, whatever the flag."""
    from streamvoiceanon_amd import infer_arvc, stream_pool

    for fn in (stream_pool.run_pool, stream_pool.SlotPool.__init__, stream_pool.SlotPool.plan):
        assert "slot_priming" not in inspect.signature(fn).parameters
    sig = inspect.signature(infer_arvc.InferenceWrapper.stream_infer_many)
    assert sig.parameters["slot_priming"].default is False
    monkeypatch.setattr(infer_arvc.E, "Batch", _FakeBatch)
    _FakeBatch.made = []
    rng = np.random.default_rng(3)
    lengths = (4, 7, 3, 5, 2)
    srcs = [rng.uniform(1, 2, N * c).astype(np.float32) for c in lengths]
    prompts = [(np.full((8, 3), u, np.int32), np.full(3, u, np.int64), np.full(192, u, np.float32), np.full((32, 128), u, np.float32))
               for u in range(len(lengths))]
    outs = {}
    for flag in (False, True):
        me = types.SimpleNamespace(SAMPLES_PER_FRAME=N, _load_src=lambda a: (a[:-1], 44100), batch=None, engine=None, delay=2,
                                   decode_chunk_frames=1)          # (_load_src drops a sample: stream_infer_many pads to whole chunks)
        outs[flag] = infer_arvc.InferenceWrapper.stream_infer_many(me, srcs, prompts, n_slots=2, noise_seeds=list(range(5)), slot_priming=flag)
    off, on = _FakeBatch.made
    assert off.kw["slot_priming"] is False and on.kw["slot_priming"] is True
    assert {k: v for k, v in off.kw.items() if k != "slot_priming"} == {k: v for k, v in on.kw.items() if k != "slot_priming"}
    assert off.calls == on.calls and sum(c[0] == "restart" for c in on.calls) == 3
    for u, c in enumerate(lengths):
        np.testing.assert_array_equal(outs[False][u], outs[True][u])
        assert outs[True][u].shape == (N * c,) and outs[True][u].min() >= 1000.0 * u
