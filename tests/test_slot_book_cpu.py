"""The host-side book of the per-slot stream state, pinned without a GPU (csrc/slot_book.h through sva_test_slot_book).

Every case runs a script of ops (begin / prefilled / step / restart / retire) through the hook and through the short model below, and the
two traces must be equal, entry by entry.  The model is written from the reference's rules (evaluations/infer_arvc.py:443-596,
modules/dual_ar_stream.py:764-837) and the engine's documented treatment of parked slots (restart and retire); it does not call
the hook:
  * a prompt of R frames is prefilled into positions 0 .. nspk + 2R - 1 (nspk = speaker prefix rows);
  * the delay fill writes 2 delay - 1 more rows -- for EVERY slot of the batch when the lock-step slots have seen `delay` content codes, for
    one slot when it is re-prefilled or activated;
  * every decoded frame advances the position by 2; a parked slot (retired, or restarted and filling its own delay) rides along;
  * a decoding slot is re-prefilled when pos // 2 >= max_seq_frames, to nspk + 2 (Rt + min(buffer_frames, nframes)) - 1, then delay-filled;
    all due slots go in one pass only if each has decoded at least `delay` frames;
  * a parked slot that would be due is rewound to nspk - 1 + 2 Rt, where its stored prompt ends; so is a slot at its restart;
  * a restarted slot counts content from its restart and is activated at the end of the step in which the count reaches the delay.
"""
import numpy as np
import pytest

from conftest import load_golden
from streamvoiceanon_amd import engine as E

BEGIN, PREFILLED, STEP, RESTART, RETIRE = 0, 1, 2, 3, 4


class Model:
    def __init__(self, B, chunk, delay, max_seq_frames, buffer_frames, window, nspk):
        self.B, self.c, self.d, self.msf, self.bf, self.win, self.nspk = B, chunk, delay, max_seq_frames, buffer_frames, window, nspk
        self.phase, self.pos, self.nf, self.nc = [1] * B, [-1] * B, [0] * B, [0] * B
        self.R, self.pending = [0] * B, [None] * B
        self.filled = False

    def _priming(self, R):
        return min(self.win - 1, R) // self.c * self.c

    def _prefill_end(self, R):
        return self.nspk + 2 * R - 1

    def run(self, op, slot, R):
        B, c, d = self.B, self.c, self.d
        redo, rewind, acts, one_pass, prime = [], [], [], -1, -1
        if op == BEGIN:
            self.filled = False
            for i in range(B):
                self.phase[i], self.nf[i], self.nc[i], self.pending[i] = 1, 0, 0, None
            prime = min(self._priming(r) for r in self.R)
        elif op == PREFILLED:
            self.R[slot], self.pos[slot] = R, self._prefill_end(R)
        elif op == RESTART:
            self.pending[slot], self.phase[slot], self.nc[slot] = R, 1, 0
            self.pos[slot] = self.nspk - 1 + 2 * self.R[slot]
        elif op == RETIRE:
            self.pending[slot], self.phase[slot] = None, 0
        elif op == STEP:
            if not self.filled:
                for i in range(B):
                    self.nc[i] += c
                lock = [i for i in range(B) if self.phase[i] == 1 and self.pending[i] is None]
                if not lock:
                    self.filled = True
                elif self.nc[lock[0]] >= d:
                    for i in range(B):
                        self.pos[i] += 2 * d - 1
                    for i in lock:
                        self.phase[i] = 2
                    self.filled = True
            else:
                for i in range(B):
                    self.nc[i] += c
                    self.pos[i] += 2 * c
                    if self.phase[i] == 2:
                        self.nf[i] += c
                    if self.pos[i] // 2 >= self.msf:
                        if self.phase[i] == 2:
                            redo.append(i)
                        else:
                            self.pos[i] = self.nspk - 1 + 2 * self.R[i]
                            rewind.append((i, self.pos[i]))
                if redo:
                    one_pass = int(all(min(self.bf, self.nf[i]) >= d for i in redo))
                for i in redo:
                    self.pos[i] = self.nspk + 2 * (self.R[i] + min(self.bf, self.nf[i])) - 1 + (2 * d - 1)
            acts = [i for i in range(B) if self.pending[i] is not None and self.phase[i] == 1 and self.nc[i] >= d]
            for i in acts:
                self.R[i], self.pending[i] = self.pending[i], None
                self.pos[i] = self._prefill_end(self.R[i]) + 2 * d - 1
                self.phase[i], self.nf[i] = 2, 0
            if acts:
                prime = self._priming(self.R[acts[0]])
        row = []
        for i in range(B):
            row += [self.phase[i], self.pos[i], self.nf[i], self.nc[i]]
        row += [int(self.filled), one_pass]
        row += [len(redo)] + redo + [-1] * (B - len(redo))
        row += [len(rewind)] + [x for p in rewind for x in p] + [-1] * (2 * (B - len(rewind)))
        row += [len(acts)] + acts + [-1] * (B - len(acts))
        row += [prime]
        return row


class Cols:
    """column indices of a trace row (include/sva.h)"""

    def __init__(self, B):
        self.B = B
        self.filled, self.one_pass, self.n_redo, self.n_rewind, self.n_act, self.prime = 4 * B, 4 * B + 1, 4 * B + 2, 5 * B + 3, 7 * B + 4, 8 * B + 5

    def pos(self, i):
        return 4 * i + 1

    def phase(self, i):
        return 4 * i

    def nframes(self, i):
        return 4 * i + 2


def both(cfg, ops):
    """-> the hook's trace, after checking it against the model's"""
    ops = [tuple(op) + (0,) * (3 - len(op)) for op in ops]
    got = E.test_slot_book(cfg, ops)
    m = Model(*cfg)
    want = np.array([m.run(*op) for op in ops], dtype=np.int32)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"first differing op {bad[0]} {ops[bad[0]]}: hook {got[bad[0]].tolist()} model {want[bad[0]].tolist()}"
    return got


def start(prompts):
    return [(PREFILLED, i, R) for i, R in enumerate(prompts)] + [(BEGIN,)]


def test_default_long_stream_reprefills_where_the_reference_does():
    """The reference's default stream of tests/golden/stream_long_reprefill.npz: the first re-prefill is planned at the end of step index 645
    (the fixture's "re-prefill at chunk 646"), it lands -- with its delay fill -- on position 313, and the stream ends where the fixture's does."""
    g = load_golden("stream_long_reprefill")
    R, d, n = int(g["prompt_frames"]), int(g["delay"]), int(g["n_chunks"])
    cfg = (1, 1, d, int(g["max_seq_frames"]), int(g["buffer_frames"]), 64, 33)
    assert (R, d, n, cfg[3], cfg[4]) == (107, 2, 672, 768, 32)
    ops = start([R]) + [(STEP,)] * n
    t = both(cfg, ops)
    C, steps = Cols(1), t[2:]
    assert int(t[0, C.pos(0)]) == 33 + 2 * 107 - 1 and int(t[1, C.prime]) == 63
    redo_at = np.nonzero(steps[:, C.n_redo] > 0)[0]
    assert redo_at.tolist() == [645]
    assert steps[645, C.one_pass] == 1 and steps[645, C.pos(0)] == 313 and steps[644, C.pos(0)] == 249 + 2 * 643
    assert steps[1, C.filled] == 1 and steps[0, C.filled] == 0 and steps[1, C.pos(0)] == 249
    assert int(steps[-1, C.pos(0)]) == int(g["final_pos"])
    assert int(steps[-1, C.nframes(0)]) == g["audio_codes"].shape[1]


def test_chunk4_two_streams():
    cfg = (2, 4, 2, 100, 32, 64, 33)
    t = both(cfg, start([40, 25]) + [(STEP,)] * 60)
    C = Cols(2)
    assert t[3, C.filled] == 1                                   # the first chunk already holds the delay
    assert (t[:, C.n_redo] > 0).sum() >= 3 and t[2, C.prime] == 24
    assert set(t[3:, C.n_redo].tolist()) >= {1}                  # the two prompts differ: they do not re-prefill together


def test_three_streams_reprefills_and_a_parked_rewind():
    cfg = (3, 1, 2, 100, 32, 64, 33)
    ops = start([20, 30, 12]) + [(STEP,)] * 10 + [(RETIRE, 2)] + [(STEP,)] * 190
    t = both(cfg, ops)
    C = Cols(3)
    assert (t[:, C.n_redo] > 0).sum() >= 6
    rew = t[t[:, C.n_rewind] > 0]
    assert len(rew) >= 2 and set(rew[:, C.n_rewind + 1].tolist()) == {2} and set(rew[:, C.n_rewind + 2].tolist()) == {33 - 1 + 2 * 12}
    assert (t[15:, C.phase(2)] == 0).all() and (t[15:, C.nframes(2)] == t[14, C.nframes(2)]).all()
    assert (t[:, [C.pos(i) for i in range(3)]] // 2 <= 100).all()


def test_restart_during_the_batch_warmup():
    cfg = (2, 1, 3, 100, 32, 64, 33)
    ops = start([20, 24]) + [(STEP,), (RESTART, 1, 18)] + [(STEP,)] * 8
    t = both(cfg, ops)
    C = Cols(2)
    s = t[5:]                                                    # the steps after the restart
    assert s[1, C.filled] == 1 and s[1, C.phase(0)] == 2 and s[1, C.phase(1)] == 1      # slot 0 fills in lock step, slot 1 on its own
    assert s[:, C.n_act].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and s[2, C.n_act + 1] == 1
    assert s[2, C.pos(1)] == 33 + 2 * 18 - 1 + 5 and s[2, C.nframes(1)] == 0 and s[2, C.prime] == 18
    assert s[3, C.nframes(1)] == 1 and s[3, C.pos(1)] == s[2, C.pos(1)] + 2


def test_two_restarts_with_overlapping_delay_phases():
    cfg = (3, 1, 3, 100, 32, 64, 33)
    ops = start([20, 24, 28]) + [(STEP,)] * 6 + [(RESTART, 0, 17), (STEP,), (RESTART, 2, 40), (STEP,), (STEP,), (STEP,), (STEP,), (STEP,)]
    t = both(cfg, ops)
    C = Cols(3)
    acts = [(k, t[k, C.n_act + 1]) for k in range(len(t)) if t[k, C.n_act] > 0]
    assert [a[1] for a in acts] == [0, 2] and acts[1][0] - acts[0][0] == 1      # one step apart, as their restarts were
    assert t[5, C.filled] == 0 and t[6, C.filled] == 1 and (t[6:, C.phase(1)] == 2).all()      # the untouched slot never leaves decoding


def test_retire_then_restart():
    cfg = (2, 1, 2, 60, 32, 64, 33)
    ops = start([20, 20]) + [(STEP,)] * 5 + [(RETIRE, 1)] + [(STEP,)] * 30 + [(RESTART, 1, 22)] + [(STEP,)] * 6
    t = both(cfg, ops)
    C = Cols(2)
    assert (t[t[:, C.n_rewind] > 0][:, C.n_rewind + 1] == 1).all() and (t[:, C.n_rewind] > 0).any()     # the retired slot is rewound, never re-prefilled
    k = len(start([20, 20])) + 5 + 1 + 30
    assert t[k, C.phase(1)] == 1 and t[k, C.pos(1)] == 33 - 1 + 2 * 20 and t[k + 2, C.n_act] == 1 and t[k + 2, C.phase(1)] == 2
    assert t[k + 2, C.pos(1)] == 33 + 2 * 22 - 1 + 3


def test_every_slot_retired_before_the_delay_fills():
    cfg = (2, 1, 3, 100, 32, 64, 33)
    ops = start([20, 24]) + [(STEP,), (RETIRE, 0), (RETIRE, 1), (STEP,), (STEP,)]
    t = both(cfg, ops)
    C = Cols(2)
    assert t[3, C.filled] == 0 and t[6, C.filled] == 1
    assert t[6, C.pos(0)] == t[0, C.pos(0)] and t[6, C.pos(1)] == t[1, C.pos(1)]        # no lock-step fill: nobody's position moved
    assert t[7, C.pos(0)] == t[0, C.pos(0)] + 2 and (t[:, C.phase(0)][4:] == 0).all()


def test_reprefill_with_fewer_decoded_frames_than_the_delay_is_not_one_pass():
    cfg = (1, 1, 2, 125, 32, 64, 33)         # prompt 107: position 249 after the delay fill, 251 // 2 = 125 after ONE frame
    t = both(cfg, start([107]) + [(STEP,)] * 5)
    C = Cols(1)
    first = int(np.nonzero(t[:, C.n_redo] > 0)[0][0])
    assert first == 4 and t[first, C.nframes(0)] == 1 and t[first, C.one_pass] == 0
    assert t[first, C.pos(0)] == 33 + 2 * (107 + 1) - 1 + 3
    assert t[first + 1, C.one_pass] == 1                          # two frames by then


@pytest.mark.parametrize("Rt,one_pass", [(1, 0), (2, 1), (3, 1)])
def test_reprefill_of_a_stored_prompt_shorter_than_the_delay_is_not_one_pass(Rt, one_pass):
    """A prompt stored truncated to Rt < delay frames (op 5: max_prompt_frames below the delay): frames Rt .. delay - 1 of the re-prefilled prompt carry
    wait4start rows (DualAR.prefill_prompt), which only the whole-prompt prefill builds -- the one-pass launchers refuse Rt < delay
    (test_gpu_step_ops.py).  The positions are the reference's either way."""
    TRUNCATED = 5
    cfg = (1, 1, 2, 30, 6, 4, 33)          # delay 2: a prompt of 3 + Rt frames; position 33 + 2 (3 + Rt) - 1 + 3 after the delay fill
    t = E.test_slot_book(cfg, [(TRUNCATED, 0, Rt), (BEGIN, 0, 0)] + [(STEP, 0, 0)] * 20)
    C = Cols(1)
    due = np.nonzero(t[:, C.n_redo] > 0)[0]
    assert due.size >= 1
    first = int(due[0])
    nf = int(t[first, C.nframes(0)])
    assert nf >= 6 and t[first - 1, C.pos(0)] + 2 >= 60
    assert (t[due, C.one_pass] == one_pass).all()
    assert t[first, C.pos(0)] == 33 + 2 * (Rt + 6) - 1 + 3          # [stored prompt, the last buffer_frames = 6 frames], then the delay fill


def test_hook_refuses_what_the_engine_refuses():
    with pytest.raises(RuntimeError):
        E.test_slot_book((1, 1, 2, 100, 32, 64, 33), [(BEGIN, 0, 0)])            # begin before every slot was prefilled
    with pytest.raises(RuntimeError):
        E.test_slot_book((1, 1, 2, 100, 32, 64, 33), [(PREFILLED, 0, 2)])        # a prompt no longer than the delay


@pytest.mark.parametrize("R,Rt,ncb,P,first,n", [(107, 107, 8, 63, 0, 63), (107, 107, 8, 63, 62, 1), (107, 90, 8, 60, 8, 4), (40, 17, 3, 16, 5, 11), (20, 20, 1, 0, 0, 0)])
def test_stored_prompt_is_truncated_and_its_tail_is_the_last_frames(R, Rt, ncb, P, first, n):
    """The stored prompt keeps the first Rt of R frames of every codebook (infer_arvc.py:469-470); the vocoder is primed with frames
    Rt - P + first .. of it (:567-571)."""
    got, stored = E.test_slot_prompt_tail(R, Rt, ncb, P, first, n)
    assert stored == (Rt, Rt, ncb * Rt, Rt - 1)
    want = np.array([[1000 * q + (Rt - P + first + k) for k in range(n)] for q in range(ncb)], dtype=np.int32).reshape(ncb, n)
    np.testing.assert_array_equal(got, want)
