"""sva_config.enc_dtype = 1: the tokenizer's content encoder on fp16 operands with fp32 accumulation.

  * the weight-streaming fp16-MFMA kernel (csrc/gemm_stream_h.hip) against float64 on the rounded operands, across its tile
    configurations, conv forms and epilogues; row-position independence; the range report;
  * the mode end to end: below batch scale (that kernel), at batch scale (the planes kernel in H1), streaming;
  * the default (enc_dtype = 0) untouched by an fp16 engine in the same process.

Yardstick Y = ENC_FP16_YARDSTICK: how far the reference's own formulation moves under torch.autocast(fp16)
(tests/test_enc_fp16_cpu.py).  End-to-end gate: max |u - u_fp32| <= 2 Y.  Why no tighter gate against the emulation: two CPU emulations of
this very mode that differ only in the accumulation precision (float32 / float64) sit 6.6e-4 = 0.6 Y apart in u -- rounding flips of
the fp16 operands cascade through the layers."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from enc_fp16_ref import ENC_FP16_YARDSTICK as Y, agreement, emulated_encode_window
from kernel_refs import round_f16
from test_gpu_kernels import digest

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# every (mt, nt, kw) the heuristic of gemm_stream_h.hip can return (stream_h_config): mt by the rows, nt by SwiGLU / the width, kw by K
CONFIGS = [(1, 1, 4), (1, 1, 8), (1, 1, 16), (2, 1, 4), (2, 1, 8), (2, 1, 16), (4, 1, 4), (4, 1, 8),
           (1, 2, 4), (1, 2, 8), (1, 2, 16), (2, 2, 4), (2, 2, 8), (4, 2, 4), (4, 2, 8)]
GELU_LIP, SILU_LIP = 1.13, 1.10          # sup |gelu'| = 1.129, sup |silu'| = 1.0998


@pytest.fixture(scope="module")
def eng16(weights0):
    from streamvoiceanon_amd import engine as E

    e = E.Engine(weights0, enc_dtype=1)
    yield e
    e.close()


# ---- (a) the kernel against float64 on the rounded operands ----------------------------------------------------------------------------
def _draw(rng, shape):
    """magnitudes in [2^-8, 2], random signs: products and operands stay clear of fp16's subnormals, which are not part of the statement"""
    return (np.exp2(rng.uniform(-8.0, 1.0, size=shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(v / np.sqrt(2.0))).numpy())


def _case(rng, B, T, N, Cin, taps=1, dil=1, stride=1, bias=True, gelu=False, gamma_res=False, swiglu=False, skip_rows=False, padded=False,
          config=(0, 0, 0)):
    """One launch through sva_test_gemm_h16 -> max error / bound over the stored elements.
    Bound before the epilogue: 2 n 2^-24 sum_k |a_k w_k| (n = taps Cin; the products of two fp16 numbers are exact in fp32, the factor 2
    covers an MFMA accumulation that does not round every add to nearest).  Linear epilogue: times |gamma|.  GELU: times its Lipschitz
    bound, + 8 ulp32 of the output.  SwiGLU: product rule on silu(g) u, + 8 ulp32 of the output."""
    from streamvoiceanon_amd import engine as E

    rows = (T - 1) * stride + (taps - 1) * dil + 1
    A, W = _draw(rng, (B, rows, Cin)), _draw(rng, (N, taps * Cin))
    b = _draw(rng, (N,)) if bias and not swiglu else None
    gm = _draw(rng, (N,)) if gamma_res else None
    rs = _draw(rng, (B, T, N)) if gamma_res else None
    Nout = N // 2 if swiglu else N
    sentinel = np.full((B, T, Nout), 777.0, np.float32)
    out, _ = E.test_gemm_h16(A, W, B, T, taps=taps, dil=dil, stride=stride, bias=b, gamma=gm, res=rs, gelu=gelu, swiglu=swiglu,
                             skip_rows=skip_rows, padded=padded, config=config, out=sentinel)
    digest("stream_h_gemm", (B, T, N, Cin, taps, dil, stride, bias, gelu, gamma_res, swiglu, skip_rows, padded, config), out)
    a16, w16 = round_f16(A).astype(np.float64), round_f16(W).astype(np.float64)
    acc, mag = np.zeros((B, T, N)), np.zeros((B, T, N))
    for tap in range(taps):
        idx = np.arange(T) * stride + tap * dil
        a, w = a16[:, idx, :], w16[:, tap * Cin:(tap + 1) * Cin]
        acc += a @ w.T
        mag += np.abs(a) @ np.abs(w).T
    tol = 2.0 * taps * Cin * 2.0 ** -24 * mag
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    if swiglu:
        g4, t4 = acc.reshape(B, T, N // 32, 2, 16), tol.reshape(B, T, N // 32, 2, 16)
        ga, up, tg, tu = g4[..., 0, :], g4[..., 1, :], t4[..., 0, :], t4[..., 1, :]
        s = ga / (1.0 + np.exp(-ga))
        ref = (s * up).reshape(B, T, Nout)
        tol = (SILU_LIP * tg * np.abs(up) + np.abs(s) * tu + SILU_LIP * tg * tu).reshape(B, T, Nout)
        tol = tol + 8.0 * ulp(ref)
    else:
        v = acc + (0.0 if b is None else b.astype(np.float64))
        if gelu:
            v, tol = _gelu64(v), GELU_LIP * tol
        if gamma_res:
            v, tol = v * gm.astype(np.float64) + rs.astype(np.float64), tol * np.abs(gm.astype(np.float64))
        ref = v
        if gelu:
            tol = tol + 8.0 * ulp(ref)
    keep = np.ones((B, T, Nout), bool)
    if skip_rows:
        keep[:, T // 4:T // 2, :] = False
        assert np.all(out[~keep] == 777.0), "skipped rows were stored"
    assert np.all(out[keep] != 777.0) and np.all(np.isfinite(out))
    return float((np.abs(out.astype(np.float64) - ref)[keep] / tol[keep]).max())


@pytest.mark.parametrize("M", [1, 17, 48, 170])
def test_kernel_vs_fp64_shapes(M, record_property):
    """Every row count x N in {16, 48 (a partial column tile), 128} x Cin in {32, 160, 1536}, Linear and 7-tap conv, the heuristic's tile."""
    rng = np.random.RandomState(100 + M)
    worst = {}
    for N in (16, 48, 128):
        for Cin, taps in ((32, 1), (160, 1), (1536, 1), (32, 7), (160, 7)):
            worst[(N, Cin, taps)] = _case(rng, 1, M, N, Cin, taps=taps)
    record_property("max_err_over_bound", {str(k): v for k, v in worst.items()})
    print("M", M, "max err / bound", max(worst.values()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("config", CONFIGS + [(0, 0, 0)])
def test_kernel_vs_fp64_tile_configurations(config, record_property):
    """Every (mt, nt, kw): B = 3 items at padded strides, 19 rows each (57 rows: partial row tiles), N = 48 (partial column tile with
    nt = 2), 7-tap conv over Cin = 160 with bias + GELU; the same with a K long enough (2 x 1536, stride 2) for the form that re-requests
    blocks; SwiGLU for the configurations that pair column tiles."""
    rng = np.random.RandomState(7)
    r = {"conv7": _case(rng, 3, 19, 48, 160, taps=7, gelu=True, padded=True, config=config),
         "long_k": _case(rng, 3, 19, 48, 1536, taps=2, stride=2, gamma_res=True, padded=True, config=config)}
    if config[1] != 1:
        r["swiglu"] = _case(rng, 3, 19, 96, 160, swiglu=True, padded=True, config=config)
    record_property("max_err_over_bound", r)
    print(config, r)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("epi", ["none", "bias", "gelu", "gamma_res", "gelu_gamma_res", "swiglu", "skip", "skip_swiglu", "stride2"])
def test_kernel_vs_fp64_epilogues(epi, record_property):
    """Every epilogue bit, the skipped history rows (sentinel rows untouched), item strides and offsets, the stride-2 two-tap conv."""
    rng = np.random.RandomState(11)
    kw = dict(none=dict(bias=False), bias=dict(), gelu=dict(gelu=True), gamma_res=dict(gamma_res=True), gelu_gamma_res=dict(gelu=True, gamma_res=True),
              swiglu=dict(swiglu=True), skip=dict(skip_rows=True, gamma_res=True), skip_swiglu=dict(skip_rows=True, swiglu=True),
              stride2=dict(taps=2, stride=2))[epi]
    r = [_case(rng, 3, 17, N, 160, padded=p, **kw) for N in (32, 128) for p in (False, True)]
    record_property("max_err_over_bound", r)
    print(epi, r)
    assert max(r) <= 1.0, r


# ---- (b) row-position independence ------------------------------------------------------------------------------------------------------
def test_row_position_independence():
    """The same 5 rows at row offsets 0, 11 and 37 of a 48-row problem, and in items 0 and 2 of B = 3: bit-identical outputs."""
    from streamvoiceanon_amd import engine as E

    rng = np.random.RandomState(3)
    Cin, N = 160, 48
    rows5 = _draw(rng, (5, Cin))
    W, b = _draw(rng, (N, Cin)), _draw(rng, (N,))
    for config in [(0, 0, 0), (1, 1, 4), (4, 2, 8)]:
        A = _draw(rng, (1, 48, Cin))
        for o in (0, 11, 37):
            A[0, o:o + 5] = rows5
        out, _ = E.test_gemm_h16(A, W, 1, 48, bias=b, gelu=True, config=config)
        for o in (11, 37):
            assert np.array_equal(out[0, o:o + 5].view(np.uint32), out[0, 0:5].view(np.uint32)), (config, o)
        A3 = _draw(rng, (3, 17, Cin))
        A3[0, 4:9] = rows5
        A3[2, 9:14] = rows5
        out3, _ = E.test_gemm_h16(A3, W, 3, 17, bias=b, gelu=True, padded=True, config=config)
        assert np.array_equal(out3[0, 4:9].view(np.uint32), out3[2, 9:14].view(np.uint32)), config
        assert np.array_equal(out3[0, 4:9].view(np.uint32), out[0, 0:5].view(np.uint32)), config


# ---- (c) range report --------------------------------------------------------------------------------------------------------------------
def test_range_check_names_the_remedy():
    """fp16's range: one operand of 1e5 makes an output non-finite; with the range check the call fails and names enc_dtype = 0 (a
    host-visible status, as sva_sync reports it for a batch); without it the call returns."""
    from streamvoiceanon_amd import engine as E

    rng = np.random.RandomState(5)
    A, W = _draw(rng, (1, 17, 64)), _draw(rng, (48, 64))
    A[0, 3, 7] = 1e5
    with pytest.raises(RuntimeError, match="enc_dtype = 0"):
        E.test_gemm_h16(A, W, 1, 17, range_check=True)
    out, _ = E.test_gemm_h16(A, W, 1, 17)
    assert not np.all(np.isfinite(out[0, 3])) and np.all(np.isfinite(out[0, 4:]))
    A[0, 3, 7] = 1.0
    out, _ = E.test_gemm_h16(A, W, 1, 17, range_check=True)
    assert np.all(np.isfinite(out))


# ---- (d) - (g) the mode end to end ----------------------------------------------------------------------------------------------------------
def _kinds(table):
    """(kernel kind, is a covered layer) per profiled conv-GEMM launch: the mel filterbank (K = 1088) is fp32 in the mode"""
    kind = (table[:, 4].astype(np.int64) // 256) - 1
    return kind, table[:, 2].astype(np.int64) != 1088


def _record(record_property, u, codes, u32, c32, uem=None):
    du = float(np.abs(u - u32).max())
    bits, whole = agreement(codes, c32)
    record_property("max_du_vs_fp32_oracle", du)
    record_property("bit_agreement", bits)
    record_property("code_agreement", whole)
    if uem is not None:
        record_property("max_du_vs_emulation", float(np.abs(u - uem).max()))
    print("max|du| vs fp32 oracle", du, "bit agreement", bits, "code agreement", whole, "vs emulation", None if uem is None else float(np.abs(u - uem).max()))
    return du


def test_encode_window_small_batch(eng16, weights0, record_property):
    """Two slots with the same 32 frames: every covered GEMM runs the fp16 weight-streaming kernel; twin slots bit-identical; u within
    2 Y of the fp32 oracle and further than 2e-5 from it (the fp16 path really ran)."""
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.synth_audio import synth_utterance

    x = synth_utterance(1000, 65536)
    b = E.Batch(eng16, n_streams=2, encode_window_frames=32)
    b.profile_gemm(True)
    codes, u = b.encode_window(np.stack([x, x]), return_u=True)
    kind, covered = _kinds(b.gemm_profile_table())
    b.close()
    assert covered.sum() >= 60 and set(kind[covered].tolist()) == {11}, sorted(set(kind[covered].tolist()))
    assert np.array_equal(u[0].view(np.uint32), u[1].view(np.uint32)) and np.array_equal(codes[0], codes[1])
    taps = {}
    xt = torch.from_numpy(x)[None]
    c32 = O.encode_window(xt, weights0, taps=taps)[0].numpy()
    _, uem = emulated_encode_window(xt, weights0)
    du = _record(record_property, u[:1], codes[:1], taps["u"].numpy(), c32, uem.numpy())
    assert 2e-5 < du <= 2 * Y, du


def test_encode_window_batch_scale_on_planes(eng16, weights0, record_property):
    """12 streams x 128 frames: the big GEMMs run the planes kernel in H1 (one fp16 plane per operand, one product), the short ones the
    fp16 weight-streaming kernel, none an fp32 kind; same gates."""
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.synth_audio import synth_utterance

    xs = [synth_utterance(1000, 262144)] + [synth_utterance(1001 + i, 262144) for i in range(1, 11)] + [synth_utterance(1000, 262144)]
    x = np.stack(xs)
    b = E.Batch(eng16, n_streams=12, encode_window_frames=128)
    b.profile_gemm(True)
    codes, u = b.encode_window(x, return_u=True)
    kind, covered = _kinds(b.gemm_profile_table())
    b.close()
    ks = set(kind[covered].tolist())
    assert ks <= {8, 10, 11} and (ks & {8, 10}), sorted(ks)          # 8 / 10: planes kernel in H1 / its LDS-DMA form; 11: gemm_stream_h.hip
    assert np.array_equal(u[0].view(np.uint32), u[11].view(np.uint32)) and np.array_equal(codes[0], codes[11])
    taps = {}
    c32 = O.encode_window(torch.from_numpy(x[:11]), weights0, taps=taps)[0].numpy()
    du = _record(record_property, u[:11], codes[:11], taps["u"].numpy(), c32)
    assert 2e-5 < du <= 2 * Y, du


def test_streaming_step_content_codes(eng16, record_property):
    """B = 1, 12 chunks through sva_step with the prompt of stream_s0: PCM finite; every content-code bit that differs from the same
    engine's encode_window of the window that chunk saw sits at |u_window| <= 2 Y, and at most 5 % of the bits are excused this way
    (the fp32 reference's own share below 2 Y is about 1 %: tests/test_enc_fp16_cpu.py)."""
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.synth_audio import frame_noise, synth_prompt, synth_utterance

    g = load_golden("stream_s0")
    useed, n_chunks, Wf = int(g["audio_seed"]), 12, 128
    ac, cc, style, timbre = synth_prompt(int(g["prompt_seed"]), int(g["prompt_frames"]))
    b = E.Batch(eng16, n_streams=1, chunk_frames=int(g["chunk"]), delay=int(g["delay"]), max_seq_frames=int(g["max_seq_frames"]),
                buffer_frames=int(g["buffer_frames"]))
    assert int(g["chunk"]) == 1
    b.prefill_prompt(0, cc, ac, style, timbre, noise_seed=useed)
    b.begin()
    src = synth_utterance(useed, 2048 * int(g["n_chunks"]))
    got, frame = [], 0
    for i in range(n_chunks):
        ns, nf = frame_noise(useed, frame)
        out = b.step(src[i * 2048:(i + 1) * 2048][None], noise=np.concatenate([ns, nf.reshape(-1)])[None])
        assert np.all(np.isfinite(out))
        got.append(int(b.tap("content_codes", (1, 1), np.int32)[0, 0]))
        if i >= int(g["delay"]):
            frame += 1
    b.close()
    # the window chunk i saw: the newest 128 frames of (silence, chunks 0 .. i); its last code
    wb = E.Batch(eng16, n_streams=1, encode_window_frames=Wf)
    hist = np.concatenate([np.zeros(Wf * 2048, np.float32), src[:n_chunks * 2048]])
    flips = excused = 0
    for i in range(n_chunks):
        end = (Wf + i + 1) * 2048
        codes, u = wb.encode_window(hist[end - Wf * 2048:end][None], return_u=True)
        diff = (int(codes[0, -1]) ^ got[i]) & 0x1FFF
        for k in range(13):                      # MSB first: bit k of the index is u[..., 12 - k]
            if (diff >> k) & 1:
                flips += 1
                assert abs(float(u[0, -1, 12 - k])) <= 2 * Y, (i, k, float(u[0, -1, 12 - k]))
                excused += 1
    wb.close()
    record_property("bits_differing", flips)
    print("streaming vs window: bits differing", flips, "of", 13 * n_chunks)
    assert excused <= 0.05 * 13 * n_chunks, excused


def test_default_engine_untouched_by_the_fp16_one(eng16, weights0):
    """An enc_dtype = 0 engine built in the same process after the fp16 one: the reference's codes exactly, u within 2e-5 (the
    dispatcher keeps no mode in thread-local or static state)."""
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.synth_audio import synth_utterance

    g = load_golden("encoder_s0")
    e = E.Engine(weights0)
    try:
        assert e.cfg.enc_dtype == 0 and eng16.cfg.enc_dtype == 1
        b = E.Batch(e, n_streams=1)
        codes, u = b.encode_window(synth_utterance(int(g["audio_seed"]), 262144)[None], return_u=True)
        b.close()
        np.testing.assert_array_equal(codes[0], g["codes"])
        assert np.abs(u[0] - g["u"]).max() <= 2e-5
    finally:
        e.close()
