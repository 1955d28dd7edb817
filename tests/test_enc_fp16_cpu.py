"""CPU pins of the yardsticks the sva_config.enc_dtype = 1 GPU tests (tests/test_gpu_enc_fp16.py) are stated in: how far the reference's
own formulation moves under torch.autocast(fp16), how far the mode's emulation (tests/enc_fp16_ref.py) moves, and how many pre-sign
values sit close enough to zero to be excused when a code bit flips."""
import numpy as np
import pytest
import torch

from enc_fp16_ref import ENC_FP16_YARDSTICK, agreement, emulated_encode_window

torch.set_grad_enabled(False)

N_SAMPLES = 262144


@pytest.fixture(scope="module")
def runs():
    """fp32 oracle, the same formulation under autocast(fp16), and the emulation of the mode: computed once for the three tests."""
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import specs
    from streamvoiceanon_amd.synth_audio import synth_utterance

    W = O.load_synth_weights(0, specs.tokenizer_specs())
    x = torch.from_numpy(np.stack([synth_utterance(1000, N_SAMPLES), synth_utterance(1001, N_SAMPLES), np.zeros(N_SAMPLES, np.float32)]))
    t32, t16 = {}, {}
    c32 = O.encode_window(x, W, taps=t32)[0].numpy()
    with torch.autocast("cpu", dtype=torch.float16):
        c16 = O.encode_window(x, W, taps=t16)[0].numpy()
    cem, uem = emulated_encode_window(x, W)
    return dict(c32=c32, u32=t32["u"].float().numpy(), c16=c16, u16=t16["u"].float().numpy(), cem=cem.numpy(), uem=uem.float().numpy())


def test_reference_formulation_under_fp16_autocast_moves_u(runs, record_property):
    """The reference runs process_one_chunk under torch.autocast(fp16) (evaluations/infer_arvc.py:493).  Y = max |du| of that run (here
    on the CPU, same cast rules: fp16 operands AND fp16 activations between layers) against the fp32 run is the yardstick of the mode's
    GPU gates.  Measured: 1.02e-3 / 1.22e-3 / 1.17e-3 on the three streams; bits 100 / 99.88 / 99.94 % equal."""
    per_stream = np.abs(runs["u16"] - runs["u32"]).reshape(3, -1).max(axis=1)
    Y = float(per_stream.max())
    bits, whole = agreement(runs["c16"], runs["c32"])
    record_property("max_du_per_stream", [float(v) for v in per_stream])
    record_property("bit_agreement", bits)
    record_property("code_agreement", whole)
    print("autocast max|du| per stream", per_stream, "bit agreement", bits, "code agreement", whole)
    assert 5e-4 <= Y <= 5e-3, Y
    # the literal the GPU tests import is this measurement (to the spread between BLAS builds of the fp16 path)
    assert 0.5 * Y <= ENC_FP16_YARDSTICK <= 2.0 * Y, (Y, ENC_FP16_YARDSTICK)


def test_emulation_of_the_mode_vs_fp32_oracle(runs, record_property):
    """The mode (fp16 operands, fp32-or-better accumulation, fp32 activations between layers) stays inside twice the reference's own
    autocast displacement and is measurably not the fp32 path.  Measured: max |du| 9.2e-4, 3 of 3328 bits flipped."""
    du = float(np.abs(runs["uem"] - runs["u32"]).max())
    bits, whole = agreement(runs["cem"], runs["c32"])
    record_property("max_du", du)
    record_property("bit_agreement", bits)
    record_property("code_agreement", whole)
    print("emulation max|du|", du, "bit agreement", bits, "code agreement", whole)
    assert 2e-5 < du <= 2 * ENC_FP16_YARDSTICK, du


def test_share_of_presign_values_near_zero(runs, record_property):
    """A code bit of the mode may differ from the fp32 code where |u_fp32| <= 2 Y.  The GPU streaming test caps the share of bits it
    excuses this way at 5 %; the fp32 reference's own share of such entries is far below the cap (measured: about 1 %)."""
    share = float((np.abs(runs["u32"]) <= 2 * ENC_FP16_YARDSTICK).mean())
    record_property("share_below_2Y", share)
    print("share of |u_fp32| <= 2Y", share)
    assert share < 0.05, share
