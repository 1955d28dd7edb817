"""CPU emulation of sva_config.enc_dtype = 1 (helper, no tests): the oracle's content encoder with every groups = 1 conv / Linear of the
tokenizer taking both operands rounded once to fp16 (round to nearest even), exact products, accumulation in float64 -- and everything
else (mel, depthwise convs, norms, attention, residuals, the BSQ projection 512 -> 13) in fp32 as the oracle has it."""
import contextlib

import torch
import torch.nn.functional as TF

# max |u_autocast - u_fp32| of the reference formulation under torch.autocast("cpu", fp16) over the three streams of
# tests/test_enc_fp16_cpu.py::test_reference_formulation_under_fp16_autocast_moves_u (its pin): the yardstick the GPU gates of the
# mode are stated in (2 Y)
ENC_FP16_YARDSTICK = 1.22e-3

BSQ_BITS = 13


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


class _Shim:
    """torch.nn.functional with fp16-operand `linear` / groups = 1 `conv1d`."""

    def __getattr__(self, name):
        return getattr(TF, name)

    @staticmethod
    def linear(x, w, b=None):
        if w.shape[0] == BSQ_BITS:                    # residual_bsq project_in: fp32 in the mode (the reference forces it, bsq.py:348-356)
            return TF.linear(x, w, b)
        y = TF.linear(_r16(x), _r16(w), None if b is None else b.to(torch.float64))
        return y.to(torch.float32)

    @staticmethod
    def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups != 1:
            return TF.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)
        y = TF.conv1d(_r16(x), _r16(w), None if b is None else b.to(torch.float64), stride=stride, padding=padding, dilation=dilation)
        return y.to(torch.float32)


@contextlib.contextmanager
def _swapped_functional():
    from oracle import sva_oracle as O

    saved = O.F
    O.F = _Shim()
    try:
        yield
    finally:
        O.F = saved


def emulated_encode_window(audio, W):
    """oracle.sva_oracle.encode_window in the mode's arithmetic -> (codes int64 [B, T], u float32 [B, T, 13])."""
    from oracle import sva_oracle as O

    taps = {}
    with _swapped_functional():
        codes = O.encode_window(audio, W, taps=taps)
    return codes[0], taps["u"]


def agreement(codes_a, codes_b, bits=BSQ_BITS):
    """(share of equal bits, share of equal whole codes) of two integer code arrays."""
    import numpy as np

    a = np.asarray(codes_a).astype(np.int64).reshape(-1)
    b = np.asarray(codes_b).astype(np.int64).reshape(-1)
    x = a ^ b
    flipped = sum(int(((x >> k) & 1).sum()) for k in range(bits))
    return 1.0 - flipped / float(a.size * bits), float((x == 0).mean())
