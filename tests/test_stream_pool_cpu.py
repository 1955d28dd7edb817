"""The slot scheduler of continuous batching (streamvoiceanon_amd/stream_pool.py) against a fake batch that records its calls:
no GPU, no engine library."""
import numpy as np
import pytest

from streamvoiceanon_amd.stream_pool import SlotPool, run_pool

N = 8          # samples per chunk of the fake


class FakeBatch:
    """Output = input + 1000 * (utterance tag of the slot's prompt); a retired slot returns zeros and must not be fed."""

    def __init__(self, n_slots, first_tags):
        self.n_slots = n_slots
        self.tag = list(first_tags) + [None] * (n_slots - len(first_tags))
        self.retired = [False] * n_slots
        self.calls = []          # ("restart", step, slot, tag) / ("retire", step, slot) / ("step", step)
        self.steps = 0

    def restart(self, slot, cc, ac, style, timbre, noise_seed=0):
        assert int(cc[0]) == int(ac[0, 0]) == int(style[0]) == int(timbre[0, 0]) == int(noise_seed)      # operands of ONE utterance
        self.calls.append(("restart", self.steps, slot, int(cc[0])))
        self.tag[slot], self.retired[slot] = int(cc[0]), False

    def retire(self, slot):
        self.calls.append(("retire", self.steps, slot))
        self.retired[slot] = True

    def step(self, x):
        assert x.shape == (self.n_slots, N)
        out = np.zeros_like(x)
        for s in range(self.n_slots):
            if self.retired[s] or self.tag[s] is None:
                assert not x[s].any(), "an idle slot was fed"
            else:
                out[s] = x[s] + 1000.0 * self.tag[s]
        self.calls.append(("step", self.steps))
        self.steps += 1
        return out


def _prompt(u):
    return (np.full((8, 3), u, np.int32), np.full(3, u, np.int64), np.full(4, u, np.float32), np.full((32, 2), u, np.float32))


def _run(lengths, n_slots):
    rng = np.random.default_rng(5)
    srcs = [rng.uniform(1, 2, n * N).astype(np.float32) for n in lengths]
    fb = FakeBatch(n_slots, list(range(min(n_slots, len(lengths)))))
    fed = []
    outs = run_pool(fb, srcs, [_prompt(u) for u in range(len(lengths))], n_slots, N, noise_seeds=list(range(len(lengths))),
                    on_step=lambda k, feeds: fed.append((k, list(feeds))))
    return srcs, fb, fed, outs


@pytest.mark.parametrize("lengths,n_slots", [([9, 14, 11, 6], 2), ([3, 1, 1, 5, 2, 2, 7], 3), ([4, 4, 4, 4], 4), ([5], 1), ([2, 6, 1], 2)])
def test_every_utterance_served_once_routed_and_trimmed(lengths, n_slots):
    srcs, fb, fed, outs = _run(lengths, n_slots)
    assert len(outs) == len(lengths)
    for u, (src, out) in enumerate(zip(srcs, outs)):
        assert out.shape == src.shape                                   # trimmed to its own chunks
        np.testing.assert_array_equal(out, src + 1000.0 * u)            # every chunk went through a slot that held ITS prompt, in order
    served = {}
    for _, feeds in fed:
        slots = [s for s, _, _ in feeds]
        assert len(set(slots)) == len(slots)
        for s, u, k in feeds:
            served.setdefault(u, []).append(k)
    assert {u: ks for u, ks in served.items()} == {u: list(range(n)) for u, n in enumerate(lengths)}      # each chunk exactly once
    restarted = [c[3] for c in fb.calls if c[0] == "restart"]
    assert restarted == list(range(min(n_slots, len(lengths)), len(lengths)))     # queue order, the first n_slots start with the batch


def test_restart_in_the_step_after_the_utterance_ends_and_retire_on_empty_queue():
    lengths, n_slots = [9, 14, 11, 6], 2
    _, fb, fed, _ = _run(lengths, n_slots)
    # slot 0: utterance 0 over steps 0..8, utterance 2 from step 9 (restart before step 9), ends after step 19 -> retired before step 20
    # slot 1: utterance 1 over steps 0..13, utterance 3 over steps 14..19 -> retired before step 20
    assert [c for c in fb.calls if c[0] != "step"] == [("restart", 9, 0, 2), ("restart", 14, 1, 3), ("retire", 20, 0), ("retire", 20, 1)] or \
        [c for c in fb.calls if c[0] != "step"] == [("restart", 9, 0, 2), ("restart", 14, 1, 3)]
    assert fb.steps == 20                                                # no step runs with every slot idle
    by_step = dict(fed)
    assert by_step[8] == [(0, 0, 8), (1, 1, 8)] and by_step[9] == [(0, 2, 0), (1, 1, 9)]
    assert by_step[13] == [(0, 2, 4), (1, 1, 13)] and by_step[14] == [(0, 2, 5), (1, 3, 0)]


def test_slots_retire_while_others_still_run():
    _, fb, fed, _ = _run([2, 6, 1], 2)
    # slot 0: utt 0 (steps 0-1), utt 2 (step 2), then the queue is empty: retired before step 3 while slot 1 runs to step 5
    assert [c for c in fb.calls if c[0] != "step"] == [("restart", 2, 0, 2), ("retire", 3, 0)]
    assert fb.steps == 6
    assert dict(fed)[4] == [(1, 1, 4)]
    assert sum(1 for c in fb.calls if c[0] == "retire" and c[2] == 0) == 1      # retired once, not every step


def test_more_slots_than_utterances():
    srcs, fb, fed, outs = _run([3, 5], 4)
    for u in range(2):
        np.testing.assert_array_equal(outs[u], srcs[u] + 1000.0 * u)
    calls = [c for c in fb.calls if c[0] != "step"]
    assert ("retire", 0, 2) in calls and ("retire", 0, 3) in calls       # the slots that never get an utterance are idled before the first step
    assert ("retire", 3, 0) in calls and not any(c[0] == "restart" for c in calls)
    assert fb.steps == 5


def test_slot_pool_state_machine():
    p = SlotPool([2, 1, 1], 2)
    assert p.start() == [(0, 0), (1, 1)]
    assert p.plan() == ([], []) and p.feeds() == [(0, 0, 0), (1, 1, 0)]
    assert p.advance() == [1]
    assert p.plan() == ([(1, 2)], []) and p.feeds() == [(0, 0, 1), (1, 2, 0)]
    assert sorted(p.advance()) == [0, 2] and p.done()
    assert p.plan() == ([], [0, 1]) and p.plan() == ([], []) and p.feeds() == []
    with pytest.raises(AssertionError):
        SlotPool([3, 0], 2)
