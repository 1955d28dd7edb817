"""Continuous batching over a queue of utterances of unequal length: which utterance sits in which slot of a running batch, when a
slot is restarted with the next one and when it is retired.  No GPU dependency: the batch is anything with `restart(slot, cc, ac, style,
timbre, noise_seed)`, `retire(slot)` and `step(pcm_in) -> pcm_out` (engine.Batch, or a recording fake in the CPU tests); with per-utterance
sampling also `set_sampling(slot, temperature, top_p)` and the same two keywords on `restart`.

Timeline of a slot: its utterance of n chunks occupies n consecutive steps (the leading zero chunks of the delay included, as
stream_infer returns them); in the step after the last one the slot carries the next utterance of the queue, or is retired when the
queue is empty.  The first `n_slots` utterances start together through the batch's own prefill_prompt + begin (the caller's job: `start()`
only says which ones)."""
from __future__ import annotations

import numpy as np


def plan_offline_waves(lengths, n_slots):
    """Offline batches (Batch.generate_many): every slot of a wave starts together and the wave lasts as long as its longest utterance, so
    the utterances are sorted by length, longest first (ties in input order), and cut into waves of at most `n_slots` -- neighbours in
    length share a wave and the frames a finished slot spends parked are as few as a cut into consecutive groups allows.
    -> per wave, the original indices of its utterances."""
    assert n_slots >= 1
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    return [order[k:k + n_slots] for k in range(0, len(order), int(n_slots))]


class SlotPool:
    """Slot assignment for `lengths[i]` chunks per utterance (all >= 1) over `n_slots` slots, in queue order."""

    def __init__(self, lengths, n_slots):
        self.lengths = [int(n) for n in lengths]
        assert all(n >= 1 for n in self.lengths), "every utterance needs at least one chunk"
        assert n_slots >= 1
        self.n_slots = int(n_slots)
        self.utt = [None] * self.n_slots        # utterance in each slot (None: idle)
        self.pos = [0] * self.n_slots           # chunks of it already fed
        self.retired = [False] * self.n_slots
        self.next = 0                           # head of the queue
        self.started = False

    def start(self):
        """-> [(slot, utterance)] that begin together; slots beyond the queue stay idle (the caller prefills them with any prompt and
        they are retired by the first plan())."""
        assert not self.started
        self.started = True
        first = []
        while self.next < len(self.lengths) and self.next < self.n_slots:
            self.utt[self.next], self.pos[self.next] = self.next, 0
            first.append((self.next, self.next))
            self.next += 1
        return first

    def done(self):
        return self.started and self.next >= len(self.lengths) and all(u is None for u in self.utt)

    def plan(self):
        """What to do BEFORE the next step: ([(slot, utterance)] to restart, [slot] to retire).  A slot whose utterance ended with the last
        step takes the head of the queue; with an empty queue it is retired (once)."""
        assert self.started
        restart, retire = [], []
        for s in range(self.n_slots):
            if self.utt[s] is not None:
                continue
            if self.next < len(self.lengths):
                self.utt[s], self.pos[s] = self.next, 0
                self.retired[s] = False
                restart.append((s, self.next))
                self.next += 1
            elif not self.retired[s]:
                self.retired[s] = True
                retire.append(s)
        return restart, retire

    def feeds(self):
        """[(slot, utterance, chunk index)] of the next step, i.e. which chunk each busy slot reads."""
        return [(s, self.utt[s], self.pos[s]) for s in range(self.n_slots) if self.utt[s] is not None]

    def advance(self):
        """The step has run: every busy slot consumed one chunk; finished utterances leave their slots.  -> [utterance] that ended."""
        ended = []
        for s in range(self.n_slots):
            if self.utt[s] is None:
                continue
            self.pos[s] += 1
            if self.pos[s] >= self.lengths[self.utt[s]]:
                ended.append(self.utt[s])
                self.utt[s] = None
        return ended


def _sampling_entry(entry):
    """None, or {temperature, top_p} of one utterance (through infer_arvc.check_sampling_kwargs) -> None or the keyword arguments of
    Batch.set_sampling / Batch.restart; per-slot sampler edits do not exist"""
    if entry is None:
        return None
    from .infer_arvc import check_sampling_kwargs

    kw = check_sampling_kwargs(dict(entry))
    if "edits" in kw:
        raise ValueError("per-utterance sampling takes temperature / top_p only (sampler edits belong to the whole batch)")
    return {"temperature": kw.get("temperature"), "top_p": kw.get("top_p")}


def run_pool(batch, sources, prompts, n_slots, samples_per_chunk, noise_seeds=None, on_step=None, sampling=None):
    """Drive `batch` (already begun with the utterances of SlotPool.start() in their slots) over `sources` (float arrays, each a whole number
    of chunks) -> per-utterance PCM, each trimmed to its own chunks.  prompts[i] = (ac, cc, style, timbre) of utterance i.
    on_step(step index, feeds) is called after every step (tests, reports).  sampling: None, or one entry per utterance -- None (the
    batch's temperature / top_p) or a dict of the two: set on the slot that takes the utterance, before the first step (batch.set_sampling)
    or with its restart (batch.restart(..., temperature=, top_p=)); a restart without an entry puts the batch's values back by itself."""
    n = int(samples_per_chunk)
    srcs = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1) for s in sources]
    assert all(s.shape[0] % n == 0 and s.shape[0] >= n for s in srcs), "sources must be whole chunks"
    pool = SlotPool([s.shape[0] // n for s in srcs], n_slots)
    seeds = list(noise_seeds) if noise_seeds is not None else [0] * len(srcs)
    outs = [np.zeros_like(s) for s in srcs]
    samp = [None] * len(srcs) if sampling is None else [_sampling_entry(e) for e in sampling]
    assert len(samp) == len(srcs), "sampling: one entry per utterance"
    for s, u in pool.start():
        if samp[u] is not None:
            batch.set_sampling(s, **samp[u])
    step = 0
    while not pool.done():
        restart, retire = pool.plan()
        for s, u in restart:
            ac, cc, style, timbre = prompts[u]
            batch.restart(s, cc, ac, style, timbre, noise_seed=seeds[u], **(samp[u] or {}))
        for s in retire:
            batch.retire(s)
        feeds = pool.feeds()
        if not feeds:
            break
        x = np.zeros((n_slots, n), np.float32)
        for s, u, k in feeds:
            x[s] = srcs[u][k * n:(k + 1) * n]
        y = np.asarray(batch.step(x)).reshape(n_slots, n)
        for s, u, k in feeds:
            outs[u][k * n:(k + 1) * n] = y[s]
        if on_step is not None:
            on_step(step, feeds)
        pool.advance()
        step += 1
    return outs
