"""Offline batches (sva_generate_many / InferenceWrapper.infer_many) without a GPU: the wave planner, the packing of the prompt passes with
their tile tables (sva_test_prefill_pack), and the exported symbol."""
import numpy as np
import pytest


def _parked(lengths, waves):
    return sum(len(w) * max(lengths[i] for i in w) - sum(lengths[i] for i in w) for w in waves)


@pytest.mark.parametrize("n_slots", [3, 8])
def test_plan_offline_waves(n_slots):
    from streamvoiceanon_amd.stream_pool import plan_offline_waves

    lengths = [5, 40, 12, 12, 3, 90, 7]
    waves = plan_offline_waves(lengths, n_slots)
    flat = [i for w in waves for i in w]
    assert sorted(flat) == list(range(len(lengths)))                       # every index exactly once
    assert all(1 <= len(w) <= n_slots for w in waves)
    assert all(lengths[a] >= lengths[b] for a, b in zip(flat, flat[1:]))   # non-increasing across the concatenated waves
    unsorted = [list(range(k, min(k + n_slots, len(lengths)))) for k in range(0, len(lengths), n_slots)]
    assert _parked(lengths, waves) <= _parked(lengths, unsorted)


def test_prefill_pack_and_tile_tables():
    from streamvoiceanon_amd import engine as E

    M, Mmax = [40, 371, 2048, 17, 16, 1, 545], 2048
    pass_of, row0_of, tiles = E.test_prefill_pack(M, Mmax)
    assert len(pass_of) == len(M) and len(tiles) == pass_of[-1] + 1
    assert pass_of[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(pass_of, pass_of[1:]))      # slots stay in order, whole
    for p in range(len(tiles)):
        mine = [i for i in range(len(M)) if pass_of[i] == p]
        assert mine and mine == list(range(mine[0], mine[-1] + 1))
        assert sum(M[i] for i in mine) <= Mmax
        assert [int(row0_of[i]) for i in mine] == [sum(M[j] for j in mine[:k]) for k in range(len(mine))]          # prefix sum inside the pass
        want = [(r, q0) for r, i in enumerate(mine) for q0 in range(0, M[i], 16)]                                   # ceil(M / 16) tiles per run, q0 from 0
        assert tiles[p] == want
        for r, q0 in tiles[p]:
            assert q0 % 16 == 0 and q0 < M[mine[r]]               # a tile starts inside its own run: none spans two runs
    # greedy: a slot opens a new pass only when it does not fit the current one
    for i in range(1, len(M)):
        if pass_of[i] != pass_of[i - 1]:
            assert row0_of[i - 1] + M[i - 1] + M[i] > Mmax
    assert list(pass_of) == [0, 0, 1, 2, 2, 2, 2]
    with pytest.raises(RuntimeError, match="sva_test_prefill_pack"):
        E.test_prefill_pack([40, 2049], Mmax)


def test_generate_many_is_exported():
    from streamvoiceanon_amd import engine as E

    assert "sva_generate_many" in E.EXPORTED_SYMBOLS
    assert hasattr(E.load_library(), "sva_generate_many") and hasattr(E.Batch, "generate_many")
