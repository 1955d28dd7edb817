"""The fast attention of ar_decode_kernel (phase FB) in its two forms, as float32 arithmetic on the host.

Codebooks 1..7 hold one head per 16-lane row and form the softmax denominator in registers, in closed form:
    inv = 1 / (((a3 + a2) + (a1 + a0))),   a_r = e_r + e_{r + 4},   e_t = exp(s_t - max s) for t <= cb, 0 beyond.
The form it replaced held key t in row t & 3 (round t >> 2), every lane of row r carrying a_r, and took 16 / wave_sum(a): the DPP tree of
wave_sum (csrc/device_util.h) doubles a_r four times inside a row (exact), row_bcast15 adds row r - 1 into rows 1 and 3, row_bcast31 adds
row 1 into rows 2 and 3, and lane 63 is read.  The model below spells those steps out on 64 lanes and must agree with the closed form bit
for bit, for every codebook and at every scale of the scores.

Codebook 0 has one key: the probability is exp(0) = 1, the denominator 16 / 16, and fmaf(1, v, 0) * 1 is v.  The kernel copies V."""
import numpy as np
import pytest

F = np.float32
LANES = np.arange(64)
N = 5000


def _dpp_wave_sum(v):
    """wave_sum of device_util.h on v [cases, 64] float32 -> [cases]: every step is one float32 addition per lane"""
    v = v.astype(F)
    v = v + v[:, LANES ^ 1]                                          # quad_perm [1,0,3,2]
    v = v + v[:, LANES ^ 2]                                          # quad_perm [2,3,0,1]
    v = v + v[:, (LANES & ~7) | (7 - (LANES & 7))]                   # row_half_mirror
    v = v + v[:, (LANES & ~15) | (15 - (LANES & 15))]                # row_mirror
    row = LANES >> 4
    src = v[:, np.maximum(row - 1, 0) * 16 + 15]                     # row_bcast15, row mask 0xa: rows 1 and 3 (the others add the 0 of `old`)
    v = v + np.where((row == 1) | (row == 3), src, F(0)).astype(F)
    src = np.broadcast_to(v[:, 31:32], v.shape)                      # row_bcast31, row mask 0xc: rows 2 and 3
    v = v + np.where(row >= 2, src, F(0)).astype(F)
    assert v.dtype == F
    return v[:, 63]


def _probs(scores, cb):
    """e_t [cases, 8] float32 of the scores [cases, 8]: positions beyond cb are masked (probability exactly 0)"""
    live = np.arange(8) <= cb
    s = np.where(live, scores, -np.inf).astype(F)
    mx = s.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(live, np.exp((s - mx).astype(F)), F(0)).astype(F)
    return e


@pytest.mark.parametrize("scale", [0.1, 1.0, 5.0, 20.0])
@pytest.mark.parametrize("cb", range(8))
def test_denominator_matches_the_dpp_tree(cb, scale):
    rng = np.random.default_rng(1000 * cb + int(scale * 10))
    e = _probs((rng.standard_normal((N, 8)) * scale).astype(F), cb)
    # the replaced form: lane of row r holds e_r (round 0) + e_{r + 4} (round 1)
    row = LANES >> 4
    lanes = (e[:, row] + e[:, row + 4]).astype(F)
    parent = (F(16) / _dpp_wave_sum(lanes)).astype(F)
    a = (e[:, :4] + e[:, 4:]).astype(F)
    closed = (F(1) / ((a[:, 3] + a[:, 2]) + (a[:, 1] + a[:, 0])).astype(F)).astype(F)
    assert closed.dtype == F and parent.dtype == F
    mismatches = int((parent.view(np.uint32) != closed.view(np.uint32)).sum())
    assert mismatches == 0, (cb, scale, mismatches)
    assert np.isfinite(closed).all() and (closed > 0).all() and (closed <= 1).all()


@pytest.mark.parametrize("scale", [0.1, 1.0, 5.0, 20.0])
def test_one_key_attention_is_v(scale):
    """cb == 0: the replaced form's output fmaf(e, v, 0) * inv with its own e and inv, against v itself"""
    rng = np.random.default_rng(int(scale * 10))
    e = _probs((rng.standard_normal((N, 8)) * scale).astype(F), 0)
    assert (e[:, 0].view(np.uint32) == F(1).view(np.uint32)).all() and not e[:, 1:].any()
    row = LANES >> 4
    inv = (F(16) / _dpp_wave_sum((e[:, row] + e[:, row + 4]).astype(F))).astype(F)
    assert (inv.view(np.uint32) == F(1).view(np.uint32)).all()
    v = (rng.standard_normal((N, 64)) * scale).astype(F)
    v[:, 0] = F(1e-42)                  # a subnormal and the extremes of the format go through unchanged too
    v[:, 1] = np.finfo(F).max
    v[:, 2] = -np.finfo(F).tiny
    # fmaf(1, v, 0): the product is exact and adding +0 changes no value (in float64: one rounding, of an exact result)
    out = ((e[:, :1].astype(np.float64) * v.astype(np.float64) + 0.0).astype(F) * inv[:, None]).astype(F)
    assert int((out.view(np.uint32) != v.view(np.uint32)).sum()) == 0
