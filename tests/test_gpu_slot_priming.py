"""Slot-local activation (sva_stream_params.slot_priming = 1): the restarted slot's vocoder state is primed in ONE T = P pass over the
batch's one-stream workspace and moved into the slot by one kernel, instead of P / chunk whole-batch vocoder steps.

Every case follows tests/test_gpu_stream_restart.py::test_restart_on_every_decode_path_twin_and_control: 17 steps, the restart before step
K0 = 5, slot 0 is the twin, the last slot(s) restarted, a control without the restart.  What is pinned, in every form the vocoder state
can take (the workspace must keep the OWNER's form, not the one B = 1, Tv = 63 would choose):
  * every other slot: PCM, codes and state bit-identical to the control;
  * the restarted slot: codes, phases and frame counts exact against its twin, PCM within the project's vocoder tolerance
    (PCM_TOL / VOC_FP16_TOL as defined in tests/test_gpu_parity.py) -- its state comes from other GEMM tilings, so bit-equality is reported
    (record_property "pcm_bit_equal", "pcm_max_abs_diff"), not asserted;
  * Batch.activations() counts the restarts as slot-local ones, none as whole-batch.
An unprimed or mis-mapped state misses the tolerance by four orders of magnitude in the first compared chunks (the first decoded chunk
after a 20-frame history differs from the same chunk after zero history by 0.67-0.80 on the CPU oracle, PCM amplitude 0.84-0.95), and
every history row is read by the very next step, so the compared chunks cover the whole state."""
import pytest
import torch

import test_gpu_stream_restart as R
from test_gpu_stream_restart import K0, _assert_twin, _assert_untouched, _prompt, _run, _utt

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PCM_TOL = 5e-5            # tests/test_gpu_parity.py: the fp32 vocoder tolerance on the tanh output
VOC_FP16_TOL = 2e-3       # tests/test_gpu_parity.py: the fp16-operand vocoder (voc_dtype = 1) against the fp32 reference
N_STEPS = 17


@pytest.fixture(scope="module")
def eng(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_voc16(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0, voc_dtype=1)
    yield e
    e.close()


@pytest.fixture
def activations(monkeypatch):
    """(n_local, n_whole) of every batch _run drives, in order, read right before the batch is closed."""
    from streamvoiceanon_amd import engine as E

    seen, close = [], E.Batch.close

    def recording_close(self):
        if self.h:
            seen.append(self.activations()[:2])
        close(self)

    monkeypatch.setattr(E.Batch, "close", recording_close)
    return seen


def _twin_case(e, B, restarted, prompt_frames=107, chunk=1, slot_priming=True, **opt):
    """Slot 0 and the `restarted` slots carry utterance A (prompt A, seed 900), the others utterance B; -> (control, restarted run)."""
    ua, ub = _utt(7801, 72), _utt(7802, 72)
    pa, pb = _prompt(2801, prompt_frames), _prompt(2802, 70)
    same = (0,) + tuple(restarted)
    prompts = [pa if s in same else pb for s in range(B)]
    seeds = [900 if s in same else 901 + s for s in range(B)]
    feeds = [[(0, ua)] if s in same else [(0, ub)] for s in range(B)]
    ctl = _run(e, B, N_STEPS, feeds, prompts, seeds, chunk=chunk, slot_priming=slot_priming, **opt)
    feeds_r = list(feeds)
    for s in restarted:
        feeds_r[s] = [(0, ua), (K0, ua)]
    run = _run(e, B, N_STEPS, feeds_r, prompts, seeds, events={K0: [("restart", s, pa, 900) for s in restarted]}, chunk=chunk,
               slot_priming=slot_priming, **opt)
    return ctl, run


def _check(ctl, run, B, restarted, path, chunk, record_property, tol=PCM_TOL):
    assert R.PCM_TOL == tol                                   # the bound _assert_twin applies to the restarted slot's PCM
    assert run["path"] == ctl["path"]
    if path is not None:
        assert run["path"] == path, "the case no longer runs the decode path it is named after"
    _assert_untouched(run, ctl, [s for s in range(B) if s not in restarted])
    for s in restarted:
        _assert_twin(run, s, K0, chunk=chunk, record_property=record_property, tag="" if len(restarted) == 1 else f"_slot{s}")


CASES = {
    # fp32 row form, the fused C = 16 level, persistent decode: the smallest batch
    "b2_rows_fused16": dict(B=2, path=1),
    # K-blocked planes and row-major planes (the forms start at 10 streams), batched persistent decode: the smallest batch whose state is planes
    "b12_planes": dict(B=12, path=2),
    # P = 60, one delay step, rows-per-frame scaling of the descriptors
    "b2_chunk4": dict(B=2, path=1, chunk=4),
    # activation out of the pipelined mode
    "b2_step_device_pipelined": dict(B=2, path=1, opt=dict(device_steps=True, pipeline=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_slot_local_activation_twin_and_control(eng, name, activations, record_property):
    cs = CASES[name]
    B, chunk = cs["B"], cs.get("chunk", 1)
    ctl, run = _twin_case(eng, B, (B - 1,), chunk=chunk, **cs.get("opt", {}))
    _check(ctl, run, B, (B - 1,), cs["path"], chunk, record_property)
    assert activations == [(0, 0), (1, 0)]
    if name != "b12_planes":
        return
    # the flag is inert until a restart, and without it the activation is the whole-batch one
    ctl0, run0 = _twin_case(eng, B, (B - 1,), slot_priming=False)
    _assert_untouched(ctl0, ctl, range(B), what="the slot_priming control")
    assert activations[2:] == [(0, 0), (0, 1)]
    _assert_untouched(run0, ctl0, range(B - 1))


def test_slot_local_activation_fp16_planes(eng_voc16, activations, record_property, monkeypatch):
    """engine voc_dtype = 1: one fp16 plane per operand"""
    monkeypatch.setattr(R, "PCM_TOL", VOC_FP16_TOL)          # _assert_twin's PCM bound for this vocoder precision; everything else stays exact
    B = 12
    ctl, run = _twin_case(eng_voc16, B, (B - 1,))
    _check(ctl, run, B, (B - 1,), 2, 1, record_property, tol=VOC_FP16_TOL)
    assert activations == [(0, 0), (1, 0)]


def test_two_slot_local_activations_in_one_step_short_prompt(eng, activations, record_property):
    """prompt of 20 frames: P = R < decode_window_frames - 1; slots 1 and 2 become due in the same step"""
    ctl, run = _twin_case(eng, 3, (1, 2), prompt_frames=20)
    _check(ctl, run, 3, (1, 2), None, 1, record_property)
    assert activations == [(0, 0), (2, 0)]
