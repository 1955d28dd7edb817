"""Per-slot sampling (sva_stream_set_sampling / sva_stream_get_sampling) without a GPU: the C ABI declares and exports the two entry points,
the continuous-batching driver hands every utterance's {temperature, top_p} to the slot that carries it, and the rows of the mixed-pair
kernel test (test_gpu_slot_sampling.py) are decidable under the pair each of them gets."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_tail_cases as G
from streamvoiceanon_amd.stream_pool import run_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8


def test_entry_points_declared_and_exported():
    from streamvoiceanon_amd import engine as E

    src = open(os.path.join(ROOT, "include", "sva.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sva_[a-z_0-9]+)\s*\(", src))
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in ("sva_stream_set_sampling", "sva_stream_get_sampling", "sva_test_sampler_rows"):
        assert name in declared, f"{name} is not declared in include/sva.h"
        assert hasattr(lib, name), f"{name} is not exported by libsva_hip.so"
        assert name in E.EXPORTED_SYMBOLS
    assert re.search(r"int\s+sva_stream_set_sampling\(sva_batch\*\s*b,\s*int slot,\s*float temperature,\s*float top_p\);", src)
    assert re.search(r"int\s+sva_stream_get_sampling\(sva_batch\*\s*b,\s*int slot,\s*float\*\s*temperature,\s*float\*\s*top_p\);", src)


class FakeBatch:
    """records set_sampling / restart / retire with the step they were made before; output = input"""

    def __init__(self, n_slots):
        self.n_slots, self.steps, self.calls = n_slots, 0, []

    def set_sampling(self, slot, temperature=None, top_p=None):
        self.calls.append(("set_sampling", self.steps, slot, temperature, top_p))

    def restart(self, slot, cc, ac, style, timbre, noise_seed=0, **kw):
        assert set(kw) <= {"temperature", "top_p"}
        self.calls.append(("restart", self.steps, slot, int(cc[0]), kw))

    def retire(self, slot):
        self.calls.append(("retire", self.steps, slot))

    def step(self, x):
        self.steps += 1
        return x.copy()


def _prompt(u):
    return (np.full((8, 3), u, np.int32), np.full(3, u, np.int64), np.full(4, u, np.float32), np.full((32, 2), u, np.float32))


def test_run_pool_hands_each_utterance_its_pair():
    lengths, n_slots = [9, 14, 11, 4, 3], 2
    sampling = [None, {"temperature": 1.0, "top_p": 0.9}, {"top_p": 0.3}, None, {"temperature": 1.3, "top_p": 0.3}]
    rng = np.random.default_rng(5)
    srcs = [rng.uniform(1, 2, n * N).astype(np.float32) for n in lengths]
    fb = FakeBatch(n_slots)
    slot_of = {}
    outs = run_pool(fb, srcs, [_prompt(u) for u in range(5)], n_slots, N, noise_seeds=list(range(5)), sampling=sampling,
                    on_step=lambda k, feeds: [slot_of.setdefault(u, s) for s, u, _ in feeds])
    for u in range(5):
        np.testing.assert_array_equal(outs[u], srcs[u])
    assert slot_of == {0: 0, 1: 1, 2: 0, 3: 1, 4: 1}         # slot 0: 9 + 11 chunks; slot 1: 14 + 4 + 3
    calls = [c for c in fb.calls if c[0] != "retire"]
    assert calls == [
        ("set_sampling", 0, 1, 1.0, 0.9),                     # before the first step, utterance 1 in slot 1; none for utterance 0 (None)
        ("restart", 9, 0, 2, {"temperature": None, "top_p": 0.3}),
        ("restart", 14, 1, 3, {}),                            # no entry: the restart alone, which puts the batch's pair back
        ("restart", 18, 1, 4, {"temperature": 1.3, "top_p": 0.3}),
    ]
    # no sampling argument: the calls of the driver as it was
    fb2 = FakeBatch(n_slots)
    run_pool(fb2, srcs, [_prompt(u) for u in range(5)], n_slots, N, noise_seeds=list(range(5)))
    assert [c for c in fb2.calls if c[0] != "retire"] == [("restart", 9, 0, 2, {}), ("restart", 14, 1, 3, {}), ("restart", 18, 1, 4, {})]


def test_run_pool_refuses_bad_entries():
    srcs = [np.ones(N, np.float32)] * 2
    with pytest.raises(TypeError):
        run_pool(FakeBatch(2), srcs, [_prompt(0), _prompt(1)], 2, N, sampling=[{"top_k": 5}, None])
    with pytest.raises(ValueError):
        run_pool(FakeBatch(2), srcs, [_prompt(0), _prompt(1)], 2, N, sampling=[None, {"suppress_tokens": [3]}])
    with pytest.raises(AssertionError):
        run_pool(FakeBatch(2), srcs, [_prompt(0), _prompt(1)], 2, N, sampling=[None])


def mixed_cases(V):
    """the rows of the per-row kernel test: (logits, noise, [(top_p, temperature)] per row) -- row r of the random rows under
    RANDOM_SETTINGS[r % 5], row r of the hard rows under HARD_SETTINGS[r % 5]"""
    L, Q = G.random_rows(V)
    L, Q = L[:G.RANDOM_ROWS], Q[:G.RANDOM_ROWS]
    T, Qh = G.hard_rows(V)
    return (("random", L, Q, [G.RANDOM_SETTINGS[r % 5] for r in range(L.shape[0])]),
            ("hard", T, Qh, [G.HARD_SETTINGS[r % 5] for r in range(T.shape[0])]))


@pytest.mark.parametrize("V", G.V_ALL)
def test_mixed_rows_are_decidable(V):
    """precondition of test_gpu_slot_sampling.py::test_sampler_kernels_per_row_pairs, which compares tokens exactly: under the pair its
    row gets, no row sits where float32 rounding inside a kernel could pick another token"""
    n = 0
    for tag, L, Q, settings in mixed_cases(V):
        for r, (tp, temp) in enumerate(settings):
            assert G.undecidable(L[r:r + 1], Q[r:r + 1], tp, temp) == [], (tag, V, r, tp, temp)
            n += 1
    assert n == G.RANDOM_ROWS + 10


def test_sampling_pairs_are_the_launchers_quotient():
    """engine.sampling_pairs forms inv_temp as the launchers do: 1.0f / max(t, 1e-5f) in float"""
    from streamvoiceanon_amd import engine as E

    got = E.sampling_pairs([(0.7, 0.7), (1.3, 0.3), (0.0, 0.0), (1e-7, 1.0)])
    f = np.float32
    want = [[f(1) / f(0.7), f(0.7)], [f(1) / f(1.3), f(0.3)], [f(1) / f(1e-5), f(0)], [f(1) / f(1e-5), f(1)]]
    assert got.dtype == np.float32 and got.shape == (4, 2)
    np.testing.assert_array_equal(got, np.array(want, np.float32))
