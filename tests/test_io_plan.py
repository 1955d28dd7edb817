"""The planner of the I/O adaptor (csrc/io/io_plan.h through sva_test_io_plan), pinned without a GPU against a restatement built here from
audio_io._sinc_resample_kernel: which taps a phase keeps, when a sample is ready, how many engine steps a call runs, both FIFO levels, and
the latency constant L with its minimality."""
import math

import numpy as np
import pytest

from streamvoiceanon_amd import audio_io
from streamvoiceanon_amd import engine as E

RATES = (8000, 16000, 22050, 32000, 44100, 48000, 96000)
CHUNKS = (1, 4)
MODEL = 44100


class Direction:
    """one direction of the resampler, restated: need[j] = last input index output j reads"""

    def __init__(self, from_rate, to_rate):
        g = math.gcd(from_rate, to_rate)
        self.orig, self.new = from_rate // g, to_rate // g
        if self.orig == self.new:
            self.width, self.taps, self.lo, self.hi = 0, 1, np.zeros(1, np.int64), np.zeros(1, np.int64)
            return
        kern, self.width = audio_io._sinc_resample_kernel(self.orig, self.new)
        self.taps = kern.shape[1]
        assert self.taps == 2 * self.width + self.orig
        # a tap at the clip of the window carries cos^2(pi / 2) ~ 4e-33 times at most 1; the weakest tap inside the clip is an input sample's
        # distance 1 / (orig * new) >= 1 / 640^2 away from it: cos^2 there is > 1e-13.  1e-25 separates the two.
        live = np.abs(kern) > 1e-25
        self.lo = live.argmax(axis=1).astype(np.int64)
        self.hi = (self.taps - 1 - live[:, ::-1].argmax(axis=1)).astype(np.int64)
        assert (np.abs(kern)[~live] < 1e-30).all()

    def need(self, n_outputs):
        j = np.arange(n_outputs, dtype=np.int64)
        return (j // self.new) * self.orig - self.width + self.hi[j % self.new]

    def ready(self, need, n):
        """outputs whose last input has arrived once n inputs have: need is sorted"""
        return np.searchsorted(need, n, side="left")


def restate(io_rate, chunk_frames, n_total):
    """ready counts for every N in 0 .. n_total: model-rate samples, steps, io-rate samples"""
    C = 2048 * chunk_frames
    din, dout = Direction(io_rate, MODEL), Direction(MODEL, io_rate)
    need_in = din.need(int(n_total * MODEL / io_rate) + 2 * din.new + 8)
    assert (np.diff(need_in) >= 0).all() and need_in[-1] >= n_total
    N = np.arange(n_total + 1, dtype=np.int64)
    M = din.ready(need_in, N)
    S = M // C
    need_out = dout.need(n_total + 2 * dout.new + 8)
    assert (np.diff(need_out) >= 0).all() and need_out[-1] >= S[-1] * C
    R = dout.ready(need_out, S * C)
    return din, dout, M, S, R


def block_lists(io_rate, chunk_frames):
    total = int(math.ceil(2.5 * 2048 * chunk_frames * io_rate / MODEL))
    rng = np.random.default_rng(io_rate + chunk_frames)
    ragged = []
    while sum(ragged) < total:
        ragged.append(int(rng.integers(1, 3000)))
    return {n: [n] * (total // n + 1) for n in (1, 480, 960, 2229)} | {"ragged": ragged}


@pytest.mark.parametrize("chunk_frames", CHUNKS)
@pytest.mark.parametrize("io_rate", RATES)
def test_plan_matches_the_restatement(io_rate, chunk_frames):
    C = 2048 * chunk_frames
    for name, blocks in block_lists(io_rate, chunk_frames).items():
        head, rows = E.test_io_plan(io_rate, chunk_frames, blocks)
        ends = np.cumsum(blocks)
        din, dout, M, S, R = restate(io_rate, chunk_frames, int(ends[-1]))
        assert (head["orig"], head["new"], head["width_in"], head["width_out"]) == (din.orig, din.new, din.width, dout.width), name
        assert head["hist_in"] >= din.taps - 1 and head["hist_out"] >= dout.taps - 1
        starts = ends - np.asarray(blocks)
        # the readiness rule and the steps of every call
        assert np.array_equal(rows[:, 0], M[ends] - M[starts]), name
        assert np.array_equal(rows[:, 1], S[ends] - S[starts]), name
        assert np.array_equal(rows[:, 2], R[ends] - R[starts]), name
        # chunk staging: what is staged and not consumed, after the call and at its fullest (before the call's steps)
        assert np.array_equal(rows[:, 3], M[ends] - S[ends] * C), name
        assert (rows[:, 3] >= 0).all() and (M[ends] - S[starts] * C <= head["nbuf"] * C).all(), name
        # one call touches the chunk being filled and the ones behind it, never more buffers than there are
        assert ((M[ends] - 1) // C - M[starts] // C + 1 <= head["nbuf"]).all(), name
        # output FIFO: never negative after the pop (no underrun), never above its capacity before it
        assert np.array_equal(rows[:, 4], R[ends] + head["L"] - ends), name
        assert (rows[:, 4] >= 0).all() and (rows[:, 4] + np.asarray(blocks) <= head["fifo_cap"]).all(), name


@pytest.mark.parametrize("chunk_frames", CHUNKS)
@pytest.mark.parametrize("io_rate", RATES)
def test_latency_is_minimal(io_rate, chunk_frames):
    """L + ready(N) >= N for every N of three periods of the counters' pattern, and L - 1 fails somewhere.  (Three, not two: the pattern repeats
    only once the first step has run, which takes a chunk at io_rate plus the filters' look-ahead -- at 22050 Hz that is just over a period, so
    two periods from zero stop a few samples short of a whole repeating one and miss its maximum.)"""
    C = 2048 * chunk_frames
    head, _ = E.test_io_plan(io_rate, chunk_frames, [1])
    g = math.gcd(io_rate, MODEL)
    orig, new = io_rate // g, MODEL // g
    period = orig * (math.lcm(new, C) // new)            # N -> N + period shifts every count by a whole number of chunks and of filter periods
    assert head["period"] == period
    _, _, M, S, R = restate(io_rate, chunk_frames, 3 * period)
    lag = np.arange(3 * period + 1, dtype=np.int64) - R
    assert head["L"] == lag.max()                        # (so L - 1 leaves the call that ends at the arg max one sample short)
    # the filter part: the same with an engine that consumes single samples
    din, dout = Direction(io_rate, MODEL), Direction(MODEL, io_rate)
    n = 4 * orig + 2048
    M1 = din.ready(din.need(int(n * MODEL / io_rate) + 2 * new + 8), np.arange(n + 1, dtype=np.int64))
    R1 = dout.ready(dout.need(n + 2 * orig + 8), M1)
    assert head["L_filter"] == (np.arange(n + 1) - R1).max()
    # each direction looks ahead by the half-width of its window, 6 / 0.99 periods of the lower of its two rates: at io_rate that is
    # 6.06 * max(1, r) samples going in and as many coming out, r = io_rate / 44100; one sample of rounding per direction
    assert head["L_filter"] <= math.ceil(2 * 6 / 0.99 * max(1.0, io_rate / MODEL)) + 2


def test_table_of_the_issue():
    """orig : new, width and taps of the five directions the feature was specified with"""
    for fr, to, want in ((48000, 44100, (160, 147, 7, 174)), (44100, 48000, (147, 160, 7, 161)), (16000, 44100, (160, 441, 7, 174)),
                         (44100, 16000, (441, 160, 17, 475)), (44100, 8000, (441, 80, 34, 509))):
        d = Direction(fr, to)
        assert (d.orig, d.new, d.width, d.taps) == want
        # ... and the planner's own tables: the header reports the input direction's orig : new and both widths, the histories hold `taps`
        head, _ = E.test_io_plan(fr if to == MODEL else to, 1, [1])
        if to == MODEL:
            assert (head["orig"], head["new"], head["width_in"], head["hist_in"]) == want
        else:
            assert (head["new"], head["orig"], head["width_out"], head["hist_out"]) == want


@pytest.mark.parametrize("io_rate", (7999, 96001, 44101, 47999, 44099, 0, -48000))
def test_unsupported_rates_are_refused(io_rate):
    with pytest.raises(RuntimeError, match="reduced by their gcd"):
        E.test_io_plan(io_rate, 1, [480])


def test_accepted_rates():
    for io_rate in (8000, 11025, 12000, 24000, 44000, 88200, 96000):
        head, _ = E.test_io_plan(io_rate, 1, [480])
        assert head["L"] >= 2047 * io_rate // MODEL
