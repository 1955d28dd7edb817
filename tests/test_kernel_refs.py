"""The float64 references of tests/kernel_refs.py against the oracle's own (fp32 torch) functions on the same inputs: the oracle is pinned
to the reference project's fixtures (test_oracle_golden.py), so this pins the per-kernel references to the same thing.  The two cannot be
equal (fp32 vs fp64); the oracle's rms_norm at 170 x 512 sits 8e-8 (relative) from its own float64 evaluation, so
max |ref64 - oracle32| <= 1e-5 max |ref64| leaves two orders of room for rounding and none for a wrong formula."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sva_oracle as O
import kernel_refs as R

torch.set_grad_enabled(False)


def _close(ref64, oracle32, what):
    ref64 = np.asarray(ref64, np.float64)
    got = np.asarray(oracle32, np.float64)
    assert ref64.shape == got.shape, (what, ref64.shape, got.shape)
    err, scale = np.abs(ref64 - got).max(), np.abs(ref64).max()
    print(what, "max err", err, "scale", scale, "ratio", err / (1e-5 * scale))
    assert err <= 1e-5 * scale, (what, err, scale)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def test_rms_norm_matches_oracle():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((170, 512)).astype(np.float32) * 3 + 0.5
    w = rng.uniform(0.5, 1.5, 512).astype(np.float32)
    _close(R.rms_norm(x, w, 1e-5), O.rms_norm(_t(x), _t(w)).numpy(), "rms_norm")
    # the float32 restatement is the same formula: it lands within the same distance
    _close(R.rms_norm(x, w, 1e-5), R.rms_norm(x, w, 1e-5, np.float32), "rms_norm f32 restatement")


def test_layer_norm_matches_oracle():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 384, 43)).astype(np.float32) * 2 - 1          # channel-first like the oracle
    w = rng.uniform(0.5, 1.5, 384).astype(np.float32)
    b = rng.standard_normal(384).astype(np.float32)
    want = O.layer_norm_c(_t(x), _t(w), _t(b)).numpy().transpose(0, 2, 1)
    _close(R.layer_norm(x.transpose(0, 2, 1), w, b, 1e-6), want, "layer_norm")


@pytest.mark.parametrize("C,T", [(128, 10), (512, 43)])
def test_dwconv7_ln_matches_convnext_block_prologue(C, T):
    rng = np.random.default_rng(C + T)
    x = rng.standard_normal((2, C, T)).astype(np.float32)
    w = rng.standard_normal((C, 1, 7)).astype(np.float32) * 0.4
    b, lw, lb = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
    y = O.causal_conv1d(_t(x), _t(w), _t(b), groups=C).transpose(1, 2)
    want = torch.nn.functional.layer_norm(y, (C,), _t(lw), _t(lb), 1e-6).numpy()
    xin = np.concatenate([np.zeros((2, 6, C), np.float32), x.transpose(0, 2, 1)], 1)       # the causal left pad as 6 history rows
    _close(R.dwconv7_ln(xin, w[:, 0, :].T, b, lw, lb, 1e-6), want, "dwconv7_ln")


@pytest.mark.parametrize("kind", ["noise", "silence", "impulse"])
def test_stft_mag_matches_oracle(kind):
    rng = np.random.default_rng(3)
    N = 8 * 512
    a = np.zeros((2, N), np.float32)
    if kind == "noise":
        a = rng.standard_normal((2, N)).astype(np.float32)
    elif kind == "impulse":
        a[0, 1700] = 1.0
        a[1, 5] = -1.0
    want = O.stft_magnitude(_t(a)).numpy().transpose(0, 2, 1)
    got = R.stft_mag(a)
    _close(got, want, "stft_mag " + kind)
    if kind == "silence":
        assert np.abs(got - 1e-3).max() < 1e-12          # sqrt(1e-6), not 0


def _bsq_weights(rng, C=512):
    return {"w": rng.standard_normal((13, C)).astype(np.float32) / np.sqrt(C), "b": rng.standard_normal(13).astype(np.float32) * 0.1}


def test_bsq_matches_oracle_tail():
    """the tail of bsq_encode (Linear 512 -> 13, L2 normalise, sign bits MSB first) and the final RMSNorm of its pre_module"""
    rng = np.random.default_rng(4)
    z = rng.standard_normal((40, 512)).astype(np.float32) * 2
    nw = rng.uniform(0.5, 1.5, 512).astype(np.float32)
    P = _bsq_weights(rng)
    zn = O.rms_norm(_t(z), _t(nw))
    u = torch.nn.functional.normalize(torch.nn.functional.linear(zn, _t(P["w"]), _t(P["b"])).float(), dim=-1)
    idx = ((u > 0).long() * 2 ** torch.arange(12, -1, -1)).sum(-1)
    zn64, u64, raw64, idx64 = R.bsq(z, nw, 1e-5, P["w"], P["b"])
    _close(zn64, zn.numpy(), "bsq zn")
    _close(u64, u.numpy(), "bsq u")
    assert np.abs(u64).min() >= 1e-4 and np.array_equal(idx64, idx.numpy())


def test_bsq_matches_oracle_bsq_encode(weights1):
    """through the oracle's own entry point: bsq_encode(return_u=True) on tokenizer weights; the reference consumes the oracle's last
    pre-norm activation, so only the fused RMSNorm + projection + normalise + bits are compared"""
    W, p = weights1, "tok.quantizer."
    rng = np.random.default_rng(5)
    feat = _t(rng.standard_normal((1, 512, 16)))
    captured = {}
    orig = O.rms_norm

    def spy(x, w, eps=1e-5):
        if w is W[p + "pre_module.norm.weight"]:
            captured["x"] = x.clone()
        return orig(x, w, eps)

    O.rms_norm = spy
    try:
        idx, u = O.bsq_encode(feat, W, return_u=True)
    finally:
        O.rms_norm = orig
    z = captured["x"][0].numpy()
    _, u64, _, idx64 = R.bsq(z, W[p + "pre_module.norm.weight"].numpy(), 1e-5, W[p + "residual_bsq.rvqs.0.project_in.weight"].numpy(),
                             W[p + "residual_bsq.rvqs.0.project_in.bias"].numpy())
    _close(u64, u[0].numpy(), "bsq_encode u")
    safe = np.abs(u64).min(-1) >= 1e-4
    assert safe.any() and np.array_equal(idx64[safe], idx[0].numpy()[safe])


def _fsq_weights(rng, G=8, gd=64):
    W = {}
    for g in range(G):
        W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_in.weight"] = _t(rng.standard_normal((4, gd)) / np.sqrt(gd))
        W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_in.bias"] = _t(rng.standard_normal(4) * 0.1)
        W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_out.weight"] = _t(rng.standard_normal((gd, 4)))
        W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_out.bias"] = _t(rng.standard_normal(gd) * 0.1)
    return W


def test_fsq_encode_decode_match_oracle():
    rng = np.random.default_rng(6)
    W = _fsq_weights(rng)
    Win = np.stack([W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_in.weight"].numpy() for g in range(8)])
    bin_ = np.stack([W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_in.bias"].numpy() for g in range(8)])
    Wout = np.stack([W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_out.weight"].numpy() for g in range(8)])
    bout = np.stack([W[f"voc.quantizer.residual_fsq.rvqs.{g}.project_out.bias"].numpy() for g in range(8)])
    z = rng.standard_normal((2, 512, 43)).astype(np.float32) * 2
    idx, margin = O.fsq_encode(_t(z), W, return_margin=True)
    codes64, margin64 = R.fsq_encode(z.transpose(0, 2, 1), Win, bin_)
    safe = margin64 >= 1e-4
    assert safe.mean() > 0.99 and np.array_equal(codes64[safe], idx.numpy()[safe])
    assert np.abs(margin64 - margin.numpy()).max() <= 1e-5
    codes = rng.integers(0, 1000, (2, 8, 43)).astype(np.int32)
    _close(R.fsq_decode(codes, Wout, bout), O.fsq_decode(torch.from_numpy(codes), W).numpy().transpose(0, 2, 1), "fsq_decode")


def test_conv_post_tanh_matches_oracle_tail():
    """hifigan's tail: silu -> causal conv (C -> 1, k = 7) -> tanh"""
    rng = np.random.default_rng(7)
    C, T, k = 16, 43, 7
    x = rng.standard_normal((2, C, T)).astype(np.float32) * 2
    w = rng.standard_normal((1, C, k)).astype(np.float32) * 0.2
    b = np.array([0.05], np.float32)
    want = torch.tanh(O.causal_conv1d(torch.nn.functional.silu(_t(x)), _t(w), _t(b)))[:, 0].numpy()
    xin = np.concatenate([np.zeros((2, k - 1, C), np.float32), x.transpose(0, 2, 1)], 1)
    _close(R.conv_post_tanh(xin, w[0].T, b), want, "conv_post_tanh")


@pytest.mark.parametrize("T", [48, 520])
def test_enc_attention_matches_one_window_transformer_layer(T):
    """one layer of the oracle's window_transformer (T = 520 crosses the 512-key window) against the same layer assembled in float64
    from the references: rms_norm -> wqkv -> enc_attention -> wo (gamma) -> SwiGLU (gamma) -> final rms_norm"""
    rng = np.random.default_rng(T)
    H, C, I = 2, 128, 256
    p, q = "t.", "t.layers.0."
    g = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    Wn = {q + "attention_norm.weight": rng.uniform(0.5, 1.5, C).astype(np.float32), q + "attention.wqkv.weight": g(3 * C, C) * 3,
          q + "attention.wo.weight": g(C, C), q + "attention_layer_scale.gamma": rng.uniform(0.5, 1.0, C).astype(np.float32),
          q + "ffn_norm.weight": rng.uniform(0.5, 1.5, C).astype(np.float32), q + "feed_forward.w1.weight": g(I, C),
          q + "feed_forward.w3.weight": g(I, C), q + "feed_forward.w2.weight": g(C, I),
          q + "ffn_layer_scale.gamma": rng.uniform(0.5, 1.0, C).astype(np.float32), p + "norm.weight": rng.uniform(0.5, 1.5, C).astype(np.float32)}
    x = rng.standard_normal((2, C, T)).astype(np.float32)
    want = O.window_transformer(_t(x), {k: _t(v) for k, v in Wn.items()}, p, n_layer=1, n_head=H).numpy().transpose(0, 2, 1)
    W = {k: v.astype(np.float64) for k, v in Wn.items()}
    xr = x.transpose(0, 2, 1).astype(np.float64)
    qkv = R.rms_norm(xr, W[q + "attention_norm.weight"], 1e-5) @ W[q + "attention.wqkv.weight"].T
    att = R.enc_attention(qkv, R.rope_table(T), H)
    xr = xr + (att @ W[q + "attention.wo.weight"].T) * W[q + "attention_layer_scale.gamma"]
    h = R.rms_norm(xr, W[q + "ffn_norm.weight"], 1e-5)
    a = h @ W[q + "feed_forward.w1.weight"].T
    f = ((a / (1 + np.exp(-a))) * (h @ W[q + "feed_forward.w3.weight"].T)) @ W[q + "feed_forward.w2.weight"].T
    xr = R.rms_norm(xr + f * W[q + "ffn_layer_scale.gamma"], W[p + "norm.weight"], 1e-5)
    _close(xr, want, f"window_transformer layer T={T}")
    if T > 512:        # the window binds: plain causal attention must NOT reproduce the oracle
        att_c = R.enc_attention(qkv, R.rope_table(T), H, window=T)
        assert np.abs(att_c - att).max() > 1e-3 * np.abs(att).max()


def test_decode_attention_and_rope_kvwrite_match_dual_ar_block():
    """DualAR._block (RMSNorm, wqkv, RoPE, cache write at pos, attention over 0 .. pos, wo + residual, SwiGLU) for rows at ragged positions
    of one stream's cache against the same block assembled in float64 from rope_kvwrite + decode_attention"""
    rng = np.random.default_rng(8)
    H, hd, S, M = 3, 64, 96, 4
    D, I = H * hd, 256
    p = "l."
    g = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    Wn = {p + "attention_norm.weight": rng.uniform(0.5, 1.5, D).astype(np.float32), p + "attention.wqkv.weight": g(3 * D, D) * 3,
          p + "attention.wo.weight": g(D, D), p + "ffn_norm.weight": rng.uniform(0.5, 1.5, D).astype(np.float32),
          p + "feed_forward.w1.weight": g(I, D), p + "feed_forward.w3.weight": g(I, D), p + "feed_forward.w2.weight": g(D, I)}
    pos = np.array([0, 63, 64, 95])
    kc0 = rng.standard_normal((H, S, hd)).astype(np.float32)
    vc0 = rng.standard_normal((H, S, hd)).astype(np.float32)
    x = rng.standard_normal((M, D)).astype(np.float32)
    me = types.SimpleNamespace(W={k: _t(v) for k, v in Wn.items()}, cfg=types.SimpleNamespace(n_head=H), hd=hd)
    kc, vc = _t(kc0).clone(), _t(vc0).clone()
    want = O.DualAR._block(me, _t(x), p, O.rope_table(S, hd), kc, vc, torch.from_numpy(pos)).numpy()
    W = {k: v.astype(np.float64) for k, v in Wn.items()}
    x64 = x.astype(np.float64)
    qkv = R.rms_norm(x64, W[p + "attention_norm.weight"], 1e-5) @ W[p + "attention.wqkv.weight"].T
    cache = np.stack([kc0, vc0])[None]                                    # [1 slot, 2, H, S, hd]
    slot = np.zeros(M, np.int64)
    qkv_r, cache_r = R.rope_kvwrite(qkv, cache, slot, pos, R.rope_table(S), H)
    # the oracle writes all M rows, then masks by position: row m sees the rows written at positions <= pos[m] -- the same cache
    att = R.decode_attention(qkv_r[:, :D], cache_r, slot, pos, H)
    x64 = x64 + att @ W[p + "attention.wo.weight"].T
    h = R.rms_norm(x64, W[p + "ffn_norm.weight"], 1e-5)
    a = h @ W[p + "feed_forward.w1.weight"].T
    x64 = x64 + ((a / (1 + np.exp(-a))) * (h @ W[p + "feed_forward.w3.weight"].T)) @ W[p + "feed_forward.w2.weight"].T
    _close(x64, want, "DualAR._block")
    _close(cache_r[0, 0], kc.numpy(), "k cache")
    _close(cache_r[0, 1], vc.numpy(), "v cache")
    untouched = np.ones(S, bool)
    untouched[pos] = False
    assert np.array_equal(cache_r[0][:, :, untouched], np.stack([kc0, vc0])[:, :, untouched].astype(np.float64))


def test_float32_restatements_stay_close():
    """bound() needs the float32 restatement to be the SAME formula: each lands within 1e-4 (relative) of its float64 twin"""
    rng = np.random.default_rng(9)
    H, T = 2, 80
    qkv = rng.standard_normal((1, T, 3 * H * 64)).astype(np.float32)
    tab = R.rope_table(T)
    a64, a32 = R.enc_attention(qkv, tab, H), R.enc_attention(qkv, tab, H, dt=np.float32)
    assert np.abs(a64 - a32).max() <= 1e-4 * np.abs(a64).max() and a32.dtype == np.float32
    w = rng.standard_normal((1, 4096)).astype(np.float32)
    s64, s32 = R.stft_mag(w), R.stft_mag(w, dt=np.float32)
    assert np.abs(s64 - s32).max() <= 1e-4 * np.abs(s64).max() and s32.dtype == np.float32
    e32 = R.e32_of(a32, a64)
    assert R.bound(e32, a64) >= 4 * e32 > 0


def test_planes_decode_layouts():
    rng = np.random.default_rng(10)
    rows, K = 6, 64
    x = rng.standard_normal((rows, K)).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    rm = np.stack([hi.reshape(-1), lo.reshape(-1)]).view(np.uint16)
    assert np.abs(R.planes_decode(rm, 2, rows, K, False) - x).max() <= 2.0 ** -21 * np.abs(x).max()
    blk = np.stack([a.reshape(rows, K // 32, 32).transpose(1, 0, 2).reshape(-1) for a in (hi, lo)]).view(np.uint16)
    assert np.array_equal(R.planes_decode(blk, 2, rows, K, True), R.planes_decode(rm, 2, rows, K, False))
    assert np.array_equal(R.planes_decode(blk, 1, rows, K, True), hi.astype(np.float64))


CONV_FORMS = [(3, 45, 64, 136, 3, 2, 1), (3, 45, 64, 136, 4, 1, 2), (2, 150, 32, 32, 7, 3, 1), (1, 37, 16, 160, 1, 1, 1)]      # B, T, Cin, N, taps, dil, stride


@pytest.mark.parametrize("B,T,Cin,N,taps,dil,stride", CONV_FORMS)
def test_conv_gemm_matches_torch_conv1d(B, T, Cin, N, taps, dil, stride):
    """conv_gemm(float64) is torch's conv1d (float64) over the rows conv_rows gathers from a padded array -- taps, dilation, stride, a front pad,
    a padded row stride and item stride -- and every epilogue stage applied in torch in the documented order"""
    rng = np.random.default_rng(11 * taps + stride)
    F = torch.nn.functional
    lda, front, tail = Cin + 16, 2, 3
    used = (T - 1) * stride + (taps - 1) * dil + 1
    rows_b = front + used + tail
    A = np.full((B, rows_b, lda), 1e4)
    x = rng.standard_normal((B, used, Cin)) + 0.1 * np.arange(Cin) / Cin
    A[:, front:front + used, :Cin] = x
    W = rng.standard_normal((N, taps * Cin)) / np.sqrt(taps * Cin)
    geo = dict(taps=taps, stride=stride, dil=dil, lda=lda, a_off=front * lda, a_bstride=rows_b * lda)
    rows = R.conv_rows(A, B, T, Cin, **geo)
    assert np.abs(rows).max() < 1e3          # no pad element was gathered
    wt = torch.from_numpy(W.reshape(N, taps, Cin).transpose(0, 2, 1).copy())

    def conv(inp):
        return F.conv1d(torch.from_numpy(inp.transpose(0, 2, 1).copy()), wt, stride=stride, dilation=dil)[:, :, :T].transpose(1, 2)

    bias, gamma = rng.standard_normal(N), rng.uniform(0.5, 1.5, N)
    res, c_in = rng.standard_normal((B, T, N)), rng.standard_normal((B, T, N))
    tb, tg, tr, tc = (torch.from_numpy(a) for a in (bias, gamma, res, c_in))
    v = conv(x)
    _close(R.conv_gemm(rows, W), v.numpy(), "conv")
    _close(R.conv_gemm(rows, W, bias=bias), (v + tb).numpy(), "bias")
    _close(R.conv_gemm(rows, W, bias=bias, act=1), F.gelu(v + tb).numpy(), "gelu")
    _close(R.conv_gemm(rows, W, bias=bias, act=1, gamma=gamma, res=res), (F.gelu(v + tb) * tg + tr).numpy(), "gamma + res")
    third = float(np.float32(1.0 / 3.0))
    _close(R.conv_gemm(rows, W, bias=bias, gamma=gamma, res=res, scale=third, c_in=c_in), (((v + tb) * tg + tr) * third + tc).numpy(), "scale + accumulate")
    _close(R.conv_gemm(rows, W, bias=bias, res=res, a_silu=True), (conv(F.silu(torch.from_numpy(x)).numpy()) + tb + tr).numpy(), "silu on load")
    Wp = np.abs(W)
    xp = np.abs(x)
    for t in (0, 1):                         # every tap row of output rows 0 and 1 is zero
        xp[:, t * stride + np.arange(taps) * dil] = 0.0
    Ap = A.copy()
    Ap[:, front:front + used, :Cin] = xp
    vp = F.conv1d(torch.from_numpy(xp.transpose(0, 2, 1).copy()), torch.from_numpy(Wp.reshape(N, taps, Cin).transpose(0, 2, 1).copy()), stride=stride,
                  dilation=dil)[:, :, :T].transpose(1, 2)
    want = torch.log(torch.clamp(vp, min=float(R.LOG_CLAMP)))
    got = R.conv_gemm(R.conv_rows(Ap, B, T, Cin, **geo), Wp, act=2)
    _close(got, want.numpy(), "log-clamp")
    assert (vp.numpy() < 1e-5).any()         # the clamp branch is taken
    if N % 32 == 0:
        g = v.reshape(B, T, N // 32, 2, 16)
        _close(R.conv_gemm(rows, W, w13=True), (F.silu(g[..., 0, :]) * g[..., 1, :]).reshape(B, T, N // 2).numpy(), "w13")
    if taps == 1:
        rw = rng.uniform(0.5, 1.5, Cin)
        xn = R.rms_norm(x[:, ::stride][:, :T], rw, 1e-5)                  # pinned to the oracle above
        _close(R.conv_gemm(rows, W, bias=bias, rms_w=rw), (torch.from_numpy(xn) @ torch.from_numpy(W).T + tb).numpy(), "fused rmsnorm")
    # the float32 restatement is the same formula
    r64, r32 = R.conv_gemm(rows, W, bias=bias, act=1, gamma=gamma, res=res), R.conv_gemm(rows, W, bias=bias, act=1, gamma=gamma, res=res, dt=np.float32)
    assert r32.dtype == np.float32 and np.abs(r64 - r32).max() <= 1e-5 * np.abs(r64).max()
    l64, l32 = got, R.conv_gemm(R.conv_rows(Ap, B, T, Cin, **geo), Wp, act=2, dt=np.float32)
    assert np.abs(l64 - l32).max() <= 1e-5 * np.abs(l64).max()


def test_conv_gemm_convnext_prologue_matches_dwconv7_ln():
    """dw = (...): the A rows are LayerNorm(dwconv7(x)) of the seven rows from the addressed one on -- dwconv7_ln (pinned above) on the same window"""
    rng = np.random.default_rng(12)
    B, T, C, N = 2, 7, 128, 136
    x = rng.standard_normal((B, T + 6, C))
    wT, db, lw, lb = rng.standard_normal((7, C)) * 0.4, rng.standard_normal(C), rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    W, bias = rng.standard_normal((N, C)) / np.sqrt(C), rng.standard_normal(N)
    rows = R.conv_rows(x, B, T, C, a_bstride=(T + 6) * C, extra_rows=6)
    want = R.dwconv7_ln(x, wT, db, lw, lb, 1e-6) @ W.T + bias
    _close(R.conv_gemm(rows, W, bias=bias, dw=(wT, db, lw, lb, 1e-6)), want, "ConvNeXt prologue")


def test_operand_splits_restate_the_kernels():
    """bf16 hi + mid + lo and fp16 hi + lo of float32 values: the parts are representable in their format and sum back to the value to the
    documented precision (gemm_split.hip: exactly; planes_split.h: 2^-22 relative inside the fp16 range)"""
    rng = np.random.default_rng(13)
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-3, 3, 4096))).astype(np.float32)
    hi, mid, lo = R.bf16_split3(x)
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))
    assert (np.abs(mid) <= np.abs(hi) * 2.0 ** -8).all() and (np.abs(lo) <= np.abs(hi) * 2.0 ** -16).all()
    h, l = R.h3_split(x)
    assert np.abs(h.astype(np.float64) + l - x).max() <= 2.0 ** -22 * np.abs(x).max()
    W = rng.standard_normal((8, 64)).astype(np.float32) * 0.03
    whi, wlo = R.weight_planes(W, 2)
    assert np.abs(whi + wlo - W).max() <= 2.0 ** -21 * np.abs(W).max()
    w1, z = R.weight_planes(W, 1)
    assert not z.any() and np.abs(w1 - W).max() <= 2.0 ** -11 * np.abs(W).max()


def test_conv_gemm_acceptance_table_matches_the_plan_check():
    """The (family, form) pairs tests/conv_gemm_cases.py lists as refused by design are exactly the pairs for which the restated plan check
    (csrc/gemm_dispatch.hip: plan_accepts) refuses EVERY plan of the family on the form's shape; each other pair has an accepted plan; and each of
    the fp32 families takes every one of E0 .. E6 on P0 -- so no GPU case of test_gpu_conv_gemm.py is skipped silently."""
    import conv_gemm_cases as G

    fam_plans = {G.SMALLM: G.SKINNY + G.SKINNY_Z, G.TILED: G.TILED_PLANS, G.RING: G.RING_PLANS, G.SPLIT: G.SPLIT_PLANS, G.STREAM: G.STREAM_PLANS}
    for form in G.FORMS:
        P = G.case(G.shape_of(form), form).problem()
        for fam, plans in fam_plans.items():
            accepted = [p for p in plans if G.plan_accepts(p, P)]
            assert bool(accepted) != ((fam, form) in G.REFUSED_BY_DESIGN), (G.FAMILY_NAME[fam], form, accepted[:3])
            if form in ("E0", "E1", "E2", "E3", "E4", "E5", "E6"):
                assert G.shape_of(form) == "P0" and accepted, (G.FAMILY_NAME[fam], form)
    # plan-level refusals of an accepted pair: SwiGLU on single column tiles, the ConvNeXt prologue beyond one 16 x 16 tile
    P5, P8 = G.case("P0", "E5").problem(), G.case("PD", "E8").problem()
    assert not G.plan_accepts((G.SMALLM, 1, 4, 1, 1), P5) and G.plan_accepts((G.SMALLM, 1, 4, 2, 1), P5) and not G.plan_accepts((G.TILED, 3, 0, 0, 1), P5)
    assert not G.plan_accepts((G.STREAM, 1, 4, 1, 1), P5) and G.plan_accepts((G.STREAM, 1, 4, 2, 1), P5)
    assert [p for p in G.SKINNY if G.plan_accepts(p, P8)] == [(G.SMALLM, 1, 4, 1, 1), (G.SMALLM, 1, 8, 1, 1), (G.SMALLM, 1, 16, 1, 1)]
    # E6: the reference has clamped elements, and no un-clamped pre-log value near 1 (where the log's absolute error is all relative error)
    m = G.case("P0", "E6")
    v = m.rows().astype(np.float64).reshape(m.B, m.T, -1) @ m.W.astype(np.float64).T
    assert (v <= 1e-5).sum() == 2 * m.N and v[v > 1e-5].min() >= 2.0


# ---- the tail of the AR decode --------------------------------------------------------------------------------------------------------
def test_every_gpu_sampler_row_is_decidable():
    """The GPU sampler tests compare tokens exactly.  That is sound only where float32 rounding inside a kernel cannot change the winner:
    kernel_refs.nucleus_token's decidability rule, asserted here over every row of every generator and seed those tests use
    (decode_tail_cases.all_sampler_cases).  A condition on the inputs, not a tolerance: no row is left out."""
    import decode_tail_cases as G
    n, worst = 0, float("inf")
    for tag, L, Q, tp, temp in G.all_sampler_cases():
        for r in range(L.shape[0]):
            _, ok, lead = R.nucleus_token(L[r], Q[r], temp, tp)
            assert ok, (tag, r, tp, temp, lead)
            n, worst = n + 1, min(worst, lead)
    print("decidable rows", n, "smallest lead", worst)
    assert n >= 960 and worst > 1 + 1e-4


def test_nucleus_token_matches_oracle_sample_token():
    """exact, on the random rows of the existing sampler test (48 per V) at its settings plus (0.999, 1.3), and with previous_tokens and
    suppress_tokens through kernel_refs.logit_edits"""
    import decode_tail_cases as G
    for V in (1000, 1024, 8191, 8192):
        L, Q = G.random_rows(V)
        for tp, temp in G.RANDOM_SETTINGS:
            for r in range(L.shape[0]):
                want = O.sample_token(_t(L[r]), _t(Q[r]), temp, tp)
                assert R.nucleus_token(L[r], Q[r], temp, tp)[0] == want, (V, tp, temp, r)
    rng = np.random.default_rng(77)
    for V in (1000, 8192):
        L, Q = G.random_rows(V)
        for r in range(12):
            prev = np.concatenate([np.argsort(-L[r])[:5], rng.integers(0, V, 30), np.argsort(-L[r])[:3]])        # duplicates included
            sup = np.argsort(-L[r])[5:8]
            want = O.sample_token(_t(L[r]), _t(Q[r]), 0.7, 0.7, torch.from_numpy(prev), 1.5, [int(s) for s in sup])
            row = R.logit_edits(L[r], prev, sup, 1.5)
            tok, ok, _ = R.nucleus_token(row, Q[r], 0.7, 0.7)
            assert tok == want, (V, r)


def test_logit_edits_matches_the_edit_part_of_token_probs():
    """token_probs with previous_tokens / suppress_tokens == token_probs of the rows logit_edits returns, bit for bit (the edit is one float32
    multiply or divide per listed token, from the original score); entries the kernel skips (negative, >= V) and the W / prev_cap clamp"""
    rng = np.random.default_rng(78)
    V = 1000
    row = (rng.standard_normal(V) * 4).astype(np.float32)
    row[7] = 0.0
    prev = np.array([3, 7, 3, 999, 500, 3, 0, 500], np.int64)
    sup = [11, 12, 999]
    for penalty in (1.5, 1.1, 3.0):
        want = O.token_probs(_t(row), 0.7, 0.7, torch.from_numpy(prev), penalty, sup).numpy()
        got = O.token_probs(_t(R.logit_edits(row, prev, sup, penalty)), 0.7, 0.7).numpy()
        assert np.array_equal(want, got), penalty
    e = R.logit_edits(row, prev, sup, 1.5)
    assert e[3] == (row[3] * np.float32(1.5) if row[3] < 0 else row[3] / np.float32(1.5)) and e[7] == 0.0 and np.isneginf(e[[11, 12, 999]]).all()
    untouched = np.setdiff1d(np.arange(V), np.concatenate([prev, sup]))
    assert np.array_equal(e[untouched], row[untouched])
    assert np.array_equal(R.logit_edits(row, [-1, V, V + 7, 3], [-5, V], 1.5), R.logit_edits(row, [3], [], 1.5))
    assert np.array_equal(R.logit_edits(row, prev, [], 1.5, W=2), R.logit_edits(row, prev[:2], [], 1.5))
    assert np.array_equal(R.logit_edits(row, prev, [], 1.5, W=100, prev_cap=4), R.logit_edits(row, prev[:4], [], 1.5))


def test_swiglu_row_map_is_the_packers_and_gemv_ref_matches_the_oracle_feed_forward():
    """Packer::w13 (csrc/packer.hip): out row 32 g + r = w1 row 16 g + r, out row 32 g + 16 + r = w3 row 16 g + r.  Restated as pack_w13; the
    rows swiglu_rows names for feature f must be w1 row f and w3 row f.  Then gemv_ref's SwiGLU and plain forms against DualAR._block's
    feed-forward on one small layer (wo = 0, so the block is x + w2(silu(w1 h) w3 h) with h = RMSNorm(x) ffn_norm)."""
    I, Dm = 64, 8
    w1 = np.arange(I * Dm, dtype=np.float32).reshape(I, Dm)
    w3 = -w1 - 1
    Wp = R.pack_w13(w1, w3)
    for g in range(I // 16):
        for r in range(16):
            assert np.array_equal(Wp[g * 32 + r], w1[g * 16 + r]) and np.array_equal(Wp[g * 32 + 16 + r], w3[g * 16 + r])
    r1, r3 = R.swiglu_rows(I)
    assert np.array_equal(Wp[r1], w1) and np.array_equal(Wp[r3], w3)
    rng = np.random.default_rng(79)
    H, hd, M, I = 1, 64, 3, 96
    D = H * hd
    p = "l."
    g = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    Wn = {p + "attention_norm.weight": np.ones(D, np.float32), p + "attention.wqkv.weight": g(3 * D, D), p + "attention.wo.weight": np.zeros((D, D), np.float32),
          p + "ffn_norm.weight": rng.uniform(0.5, 1.5, D).astype(np.float32), p + "feed_forward.w1.weight": g(I, D) * 2, p + "feed_forward.w3.weight": g(I, D) * 2,
          p + "feed_forward.w2.weight": g(D, I)}
    x = rng.standard_normal((M, D)).astype(np.float32)
    me = types.SimpleNamespace(W={k: _t(v) for k, v in Wn.items()}, cfg=types.SimpleNamespace(n_head=H), hd=hd)
    kc, vc = torch.zeros(H, 8, hd), torch.zeros(H, 8, hd)
    want = O.DualAR._block(me, _t(x), p, O.rope_table(8, hd), kc, vc, torch.arange(M)).numpy()
    act = R.gemv_ref(x, R.pack_w13(Wn[p + "feed_forward.w1.weight"], Wn[p + "feed_forward.w3.weight"]), norm_w=Wn[p + "ffn_norm.weight"], eps=1e-5, swiglu=True)
    _close(R.gemv_ref(act, Wn[p + "feed_forward.w2.weight"], res=x), want, "gemv_ref: SwiGLU, then plain with a residual")
    # fp16 weights: the reference runs on the rounded weights
    Wh = g(5, D)
    assert np.array_equal(R.gemv_ref(x, Wh, half=True), R.gemv_ref(x, R.round_f16(Wh)))
    # bias, and the float32 restatement within the same distance
    b = g(5)
    _close(R.gemv_ref(x, Wh, norm_w=Wn[p + "ffn_norm.weight"], bias=b), (O.rms_norm(_t(x), _t(Wn[p + "ffn_norm.weight"])) @ _t(Wh).T + _t(b)).numpy(), "gemv_ref: norm + bias")
    _close(R.gemv_ref(x, Wh, norm_w=Wn[p + "ffn_norm.weight"], bias=b), R.gemv_ref(x, Wh, norm_w=Wn[p + "ffn_norm.weight"], bias=b, dt=np.float32), "gemv_ref f32 restatement")


def test_history_ring_and_embedding_refs():
    x = np.arange(2 * 7 * 3, dtype=np.float32).reshape(2, 7, 3)
    s = R.shift_history(x, 4, 3)
    assert np.array_equal(s[:, :4], x[:, 3:7]) and np.array_equal(s[:, 4:], x[:, 4:])
    s = R.shift_history(x, 5, 2)                                           # overlap: the source rows are the ORIGINAL ones
    assert np.array_equal(s[:, :5], x[:, 2:7])
    ring = np.zeros((2, 15), np.float32)
    for step in range(7):                                                  # the reference shifts the window left and appends the chunk
        ring = R.ring_write(ring, np.full((2, 3), step + 1, np.float32), step)
    assert np.array_equal(R.ring_to_window(ring, (7 * 3) % 15)[0], np.repeat(np.arange(3, 8, dtype=np.float32), 3))
    table = np.random.default_rng(80).standard_normal((8 * 10, 5)).astype(np.float32)
    codes = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [9, 0, 9, 0, 9, 0, 9, 0]])
    want = torch.stack([_t(table)[torch.from_numpy(codes[:, i]) + 10 * i] for i in range(8)], 0).sum(0).numpy()      # BaseTransformer.embed
    _close(R.audio_embed(table, codes, 10), want, "audio_embed")


# =====================================================================================================================================
# the chunk step's bookkeeping references (test_gpu_step_ops.py): integer / copy models, pinned EXACTLY to the sequences the oracle builds
# =====================================================================================================================================
def _int_tables(rng, dim, n_content=40):
    """small-integer tables: every sum of eight entries is exact in float32 in any order, so `exactly` does not depend on how torch orders a sum"""
    g = lambda *s: rng.integers(-8, 9, s).astype(np.float32)
    return {"arvc.embedding.weight": _t(g(n_content, dim)), "arvc.decoder.model.codebook_embeddings.weight": _t(g(8 * 1000, dim)),
            "arvc.decoder.wait4start_embedding.weight": _t(g(8, dim)), "arvc.context_in.weight": _t(g(dim, 4)), "arvc.context_in.bias": _t(g(dim)),
            "arvc.style_in.weight": _t(g(dim, 4)), "arvc.style_in.bias": _t(g(dim))}


class _Rings:
    """the histories as the engine keeps them: rings of `cap` entries and their counters, the stored prompt's last max_delay audio frames"""

    def __init__(self, cap, ref_audio_stored, md=8):
        self.cap, self.md = cap, md
        self.content, self.pred = np.full((1, cap), -1, np.int64), np.full((1, 8, cap), -1, np.int64)
        self.ncontent, self.nframes = np.zeros(1, np.int64), np.zeros(1, np.int64)
        Rt = ref_audio_stored.shape[1]
        self.ref_tail = np.full((1, 8, md), 999, np.int64)          # (right-aligned; a shorter prompt leaves the front unset: 999 must never be read)
        for j in range(md):
            if Rt - md + j >= 0:
                self.ref_tail[0, :, j] = ref_audio_stored[:, Rt - md + j]


@pytest.mark.parametrize("delay,max_prompt_frames,cap", [(2, 8, 16), (1, 256, 16), (8, 9, 32), (2, 1, 16), (3, 2, 16)])
def test_row_builder_refs_are_the_oracles_sequences(delay, max_prompt_frames, cap, monkeypatch):
    """DualAR.prefill_prompt, prefill_src_condition4delay and the re-prefill branch of StreamSession.process_one_chunk hand slow_forward their
    (seq, pos); the references rebuild every such sequence from the rings (capacity 16 / 32: they wrap many times), the counters and ref_tail.
    Also holds the premise of the one-pass re-prefill -- the rows of the stored prompt are the ones the first prefill wrote -- and, for the last two
    cases (a stored prompt shorter than the delay), that the rows of frames Rt .. d - 1 are wait4start rows, which ref_tail never feeds."""
    rng = np.random.default_rng(100 * delay + max_prompt_frames)
    dim, NCt, bf, max_seq_frames, Rp = 768, 40, (6 if delay <= 3 else 12), (41 if delay <= 3 else 53), 10          # (an odd period between re-prefills: the windows meet every ring phase)
    W = _int_tables(rng, dim, NCt)
    calls = []

    def slow_forward(self, x, pos):
        calls.append((x.numpy().copy(), pos.numpy().copy()))
        return torch.zeros(dim), torch.zeros(8192)

    def decode_tokens(self, x, pos, noise_slow, noise_fast, forced=None):
        calls.append((x.numpy().copy(), pos.numpy().copy()))
        return dict(semantic=0, codes=torch.from_numpy(rng.integers(0, 1000, 8).astype(np.int32)), hidden=None, logits=None, fast_logits=None)

    monkeypatch.setattr(O.DualAR, "slow_forward", slow_forward)
    monkeypatch.setattr(O.DualAR, "decode_tokens", decode_tokens)
    cc, ac = rng.integers(0, NCt, Rp), rng.integers(0, 1000, (8, Rp))
    style, timbre = _t(rng.integers(-2, 3, 4)), _t(rng.integers(-2, 3, (32, 4)))
    sess = O.StreamSession(W, torch.from_numpy(cc), torch.from_numpy(ac), style, timbre, noise_fn=lambda f: (None, None), delay=delay,
                           max_prompt_frames=max_prompt_frames, max_seq_frames=max_seq_frames, buffer_frames=bf)
    ce, cbe, w4s = (W[k].numpy() for k in ("arvc.embedding.weight", "arvc.decoder.model.codebook_embeddings.weight", "arvc.decoder.wait4start_embedding.weight"))
    nspk, Rt = 33, min(Rp, max_prompt_frames)
    # the prompt prefill: the UNTRUNCATED prompt
    seq0, pos0 = calls.pop(0)
    rows, cre = R.prompt_rows(ce, cbe, w4s, cc, ac, delay, 1000)
    assert np.array_equal(seq0[nspk:], rows) and np.array_equal(pos0, np.arange(nspk + 2 * Rp))
    assert np.array_equal(sess.ar.cached_ref_emb.numpy(), cre)
    rings = _Rings(cap, ac[:, :Rt])
    last_pos, cached_ref = np.array([nspk + 2 * Rp - 1]), cre[None].copy()
    n_re = n_fill = 0
    straddles = dict(content=0, pred=0, fill=0)
    for step in range(270):          # (enough re-prefills for their windows to meet every phase of the ring)
        code = int(rng.integers(0, NCt))
        before = sess.n_reprefill
        sess.process_one_chunk(torch.zeros(1, 2048), content_override=torch.tensor([code]), vocode=False)
        rings.content, rings.ncontent = R.ring_append(rings.content, rings.ncontent, np.array([[code]]))
        if rings.ncontent[0] < delay:
            assert not calls
            continue

        def check_fill():
            nonlocal last_pos, n_fill
            seq, pos = calls.pop(0)
            x, so, po, cna = R.delayfill_rows(ce, rings.content, rings.ncontent, np.pad(cached_ref, ((0, 0), (0, 8 - delay), (0, 0))), last_pos, delay, [0])
            assert np.array_equal(seq, x) and np.array_equal(pos, po) and not so.any()
            assert np.array_equal(sess.ar.cached_new_audio_emb.numpy(), cna)
            lo, hi = int(rings.ncontent[0]) - delay, int(rings.ncontent[0])
            straddles["fill"] += lo // cap != (hi - 1) // cap
            last_pos = last_pos + 2 * delay - 1
            n_fill += 1
            return cna

        if rings.ncontent[0] == delay:
            cna = check_fill()
            assert not calls
            continue
        # one decoded frame: decode_one's two rows, then the frame's codes enter the prediction ring
        seq, pos = calls.pop(0)
        x, so, po, _ = R.prepare_step(cna, ce, np.array([[code]]), 0, last_pos, np.zeros((1, 1), np.int64), 0)
        assert np.array_equal(seq, x) and np.array_equal(pos, po)
        tok = sess.pred_codes[:, -1].numpy()[None]
        last_pos, rings.nframes, rings.pred, _ = R.finish_frame(tok, last_pos, rings.nframes, rings.pred, np.zeros((1, 8, 1), np.int64), 0, 2)
        cna = R.audio_embed(cbe, tok, 1000)
        if sess.n_reprefill == before:
            assert np.array_equal(sess.ar.cached_new_audio_emb.numpy(), cna) and sess.ar.last_pos == last_pos[0] and not calls
            continue
        # the re-prefill: [stored prompt, the last min(bf, frames) frames]; the one-pass form builds the rows behind the stored prompt only
        n_re += 1
        nf, ncon = int(rings.nframes[0]), int(rings.ncontent[0])
        na = min(bf, nf)
        assert na >= delay
        seq, pos = calls.pop(0)
        assert np.array_equal(seq[:nspk + 2 * Rt], seq0[:nspk + 2 * Rt]), "the stored prompt's rows are the first prefill's"
        x, so, po = R.reprefill_rows(ce, cbe, w4s, rings.content, rings.pred, rings.ref_tail, [0], [Rt], [nf], [na], [ncon], delay, 1000, nspk)
        assert np.array_equal(seq[nspk + 2 * Rt:], x) and np.array_equal(pos[nspk + 2 * Rt:], po) and not so.any()
        emb, lp = R.reprefill_finish(cbe, rings.pred, rings.ref_tail, [0], [Rt], [nf], [na], delay, 1000, nspk)
        assert np.array_equal(sess.ar.cached_ref_emb.numpy(), emb[0]) and lp[0] == len(pos) - 1
        straddles["content"] += (ncon - delay - na) // cap != (ncon - delay - 1) // cap
        straddles["pred"] += (nf - na) // cap != (nf - 1) // cap
        last_pos, cached_ref = lp, emb
        cna = check_fill()
        assert not calls and sess.ar.last_pos == last_pos[0]
    assert n_re >= 5 and n_fill == n_re + 1 and straddles["content"] >= 1 and straddles["pred"] >= 1 and (delay < 3 or straddles["fill"] >= 1), (n_re, n_fill, straddles)


def test_step_ops_cases_hold_their_preconditions():
    """every case of the GPU tests indexes inside its arrays (the hook refuses anything else), no generator is left out, every kernel of the hook has
    cases, and the ring counters really sit where their names say: each access ends before a multiple of the capacity, on it, across it and far above it"""
    import step_ops_cases as S
    from streamvoiceanon_amd import engine as E
    cases = S.all_cases()
    seen = {}
    for c in cases:
        S.validate(c)
        seen.setdefault(c["op"], []).append(c)
    assert set(seen) == set(E.STEP_OPS), set(E.STEP_OPS) ^ set(seen)
    assert len({c["id"] for c in cases}) == len(cases)

    def classes(cap, spans):
        got = set()
        for lo, hi in spans:          # entries [lo, hi)
            if lo // cap != (hi - 1) // cap:
                got.add("straddles")
            elif hi % cap == 0:
                got.add("ends on")
            elif hi % cap == cap - 1:
                got.add("ends before")
            if lo >= 4 * cap:
                got.add("far above")
        return got

    for cap in S.CAPS:
        spans = {"ar_finish_frame": [], "append_content": [], "put_codes": [], "build_delayfill": [], "reprefill content": [], "reprefill pred": []}
        for c in cases:
            d, a = c["desc"], c["arrays"]
            if c["op"] == "ar_finish_frame" and d[2] == cap:
                spans[c["op"]] += [(n, n + 1) for n in a[2]]
            elif c["op"] == "append_content" and d[3] == cap:
                spans[c["op"]] += [(n, n + d[2]) for n in a[2]]
            elif c["op"] == "put_codes" and d[3] == cap:
                spans[c["op"]] += [(n, n + d[2]) for n in a[3]]
            elif c["op"] == "build_delayfill" and d[4] == cap:
                spans[c["op"]] += [(a[2][b] - d[2], a[2][b]) for b in a[5]]
            elif c["op"] == "build_reprefill" and d[7] == cap:
                spans["reprefill content"] += [(nc - d[2] - na, nc - d[2]) for na, nc in zip(a[3], a[4])]
                spans["reprefill pred"] += [(nf - na, nf) for nf, na in zip(a[2], a[3])]
        for what, sp in spans.items():
            want = {"ends on", "ends before", "far above"} | ({"straddles"} if max(hi - lo for lo, hi in sp) > 1 else set())
            assert classes(cap, sp) >= want, (cap, what, classes(cap, sp))
    # re-prefill: na = d and na = the buffer, 1 / 3 / 128 slots, slots out of order
    re = [c for c in seen["build_reprefill"]]
    assert {c["desc"][1] for c in re} >= {1, 3, 128}
    assert any((c["arrays"][3] == c["desc"][2]).any() and (c["arrays"][3] > c["desc"][2]).any() for c in re)
    assert any(np.any(np.diff(c["arrays"][0]) < 0) for c in re)
    arms = set()
    for c in seen["history_rows_move"]:
        d = c["desc"]
        arms |= {S.move_arm(d[4 + 5 * i], d[5 + 5 * i], d[6 + 5 * i], d[1], d[7 + 5 * i], d[8 + 5 * i]) + (" odd length" if d[7 + 5 * i] * d[8 + 5 * i] % 4 else "") for i in range(d[0])}
    assert arms >= {"float4", "scalar", "scalar odd length"}, arms
    voc = S.voc_cases()
    for c in voc:
        S.validate_voc(c)
    assert {c["C"] for c in voc} == {16, 32} and {c["Tl"] for c in voc} >= set(S.VOC_TL) and {c["frames_done"] for c in voc} == {0, 1, 5}


def test_mean3_and_copy_refs():
    a, b, c = (np.random.default_rng(i).standard_normal(50).astype(np.float32) for i in range(3))
    want = torch.stack([_t(a), _t(b), _t(c)]).mean(0).numpy()          # ParallelBlock: torch.stack([...]).mean(0)
    got = R.mean3(a, b, c)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= 2 * R.ulp32(np.abs(want).max())
    tok = np.arange(2 * 9 * 4, dtype=np.float32).reshape(2, 9, 4)
    out = R.copy_tokens(tok, np.full((2, 5, 4), -1.0, np.float32), 2, 6, 1)
    assert np.array_equal(out[:, :2], tok[:, :2]) and np.array_equal(out[:, 4], tok[:, 8]) and (out[:, 2:4] == -1).all()


def _oracle_level(x_ct, W, bias, dil):
    """the inner loop of O.hifigan over one level's input [B, C, T]: the three ResBlock1 branches, before their mean"""
    out = []
    for br, k in enumerate(R.VOC_LEVEL_K):
        y = x_ct
        for j, dl in enumerate(dil):
            w1 = _t(W[br][2 * j]).reshape(-1, k, x_ct.shape[1]).permute(0, 2, 1).contiguous()          # [Cout][k Cin] tap-major -> torch's [Cout, Cin, k]
            w2 = _t(W[br][2 * j + 1]).reshape(-1, k, x_ct.shape[1]).permute(0, 2, 1).contiguous()
            t = O.causal_conv1d(F.silu(y), w1, _t(bias[br][2 * j]), dilation=dl)
            t = O.causal_conv1d(F.silu(t), w2, _t(bias[br][2 * j + 1]), dilation=dl)
            y = t + y
        out.append(y.permute(0, 2, 1).numpy())
    return np.stack(out)


@pytest.mark.parametrize("C", [16, 32])
def test_voc_level_matches_the_oracles_resblock_loop(C):
    """a window that starts at the stream start (the history rows hold NaN: never read), and the continuation window whose history is the previous
    window's tail, against the oracle's causal_conv1d + F.silu loop over the whole stream"""
    import step_ops_cases as S
    rng = np.random.default_rng(C)
    W, bias = S.voc_weights(C)
    B, T1, T2, H = 2, 200, 77, S.RF_MAX
    x = rng.standard_normal((B, T1 + T2, C)).astype(np.float32)
    want = _oracle_level(_t(x).permute(0, 2, 1), W, bias, S.DIL)
    first = np.concatenate([np.full((B, H, C), np.nan, np.float32), x[:, :T1]], axis=1)
    got1 = R.voc_level(first, W, bias, S.DIL, 0)
    _close(got1, want[:, :, :T1], "voc_level at the stream start")
    got2 = R.voc_level(x[:, T1 - H:], W, bias, S.DIL, T1)
    _close(got2, want[:, :, T1:], "voc_level continuation")
    # a stream start inside the history: 30 stream rows in front of the window
    part = np.concatenate([np.full((B, H - 30, C), np.nan, np.float32), x[:, :30 + T2]], axis=1)
    _close(R.voc_level(part, W, bias, S.DIL, 30), want[:, :, 30:30 + T2], "voc_level, stream start inside the history")
    _close(got1, R.voc_level(first, W, bias, S.DIL, 0, dt=np.float32), "voc_level f32 restatement")


@pytest.mark.parametrize("C", [16, 32])
def test_voc_conv_ref_matches_conv1d_and_the_oracles_resblock_step(C):
    """voc_conv_ref over dense rows with its history in front against torch's conv1d in float64 over the left-padded stream, for every (taps,
    dilation) of the engine and the edge forms of the GPU test; then c1 and c2 chained with the residual against one ResBlock1 step of the oracle
    (causal_conv1d(silu(.)) twice, + y)"""
    rng = np.random.default_rng(40 + C)
    B, T = 2, 70
    for taps, dil in [(3, 1), (7, 3), (11, 5), (1, 2), (2, 7), (6, 10)]:
        padL, a_row0 = (taps - 1) * dil, 4
        x = rng.standard_normal((B, T, C))
        W = rng.standard_normal((C, taps * C)) / np.sqrt(taps * C)
        bias, res = rng.standard_normal(C), rng.standard_normal((B, T, C))
        rows = np.concatenate([np.full((B, a_row0, C), np.nan), np.zeros((B, padL, C)), x, np.full((B, 3, C), np.nan)], axis=1)     # zero history = the left pad
        v, s = R.voc_conv_ref(rows, W, bias, res, taps, dil, a_row0=a_row0, T=T)
        w_t = torch.from_numpy(W).reshape(C, taps, C).permute(0, 2, 1).contiguous()                                                # [Cout, Cin, k]
        want = F.conv1d(F.pad(torch.from_numpy(x).permute(0, 2, 1), (padL, 0)), w_t, torch.from_numpy(bias), dilation=dil).permute(0, 2, 1).numpy() + res
        assert np.abs(v - want).max() <= 1e-12 * np.abs(want).max(), (taps, dil)
        assert np.abs(s - F.silu(torch.from_numpy(want)).numpy()).max() <= 1e-12 * np.abs(want).max()
        v32, s32 = R.voc_conv_ref(rows, W, bias, res, taps, dil, a_row0=a_row0, T=T, dt=np.float32)
        assert v32.dtype == np.float32 and s32.dtype == np.float32
        _close(v, v32, "voc_conv_ref f32 restatement")
        _close(s, s32, "voc_conv_ref silu f32 restatement")
    # one ResBlock1 step: t = c1(silu(y)); y' = c2(silu(t)) + y.  History rows are zero = the oracle's left pad (silu(0) = 0)
    taps, dil = 7, 3
    padL = (taps - 1) * dil
    y = rng.standard_normal((B, T, C)).astype(np.float32)
    W1, W2 = (rng.standard_normal((C, taps * C)).astype(np.float32) / np.float32(np.sqrt(taps * C)) for _ in range(2))
    b1, b2 = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
    hist = np.zeros((B, padL, C))
    _, st = R.voc_conv_ref(np.concatenate([hist, R.silu(y)], axis=1), W1, b1, None, taps, dil)
    v, _ = R.voc_conv_ref(np.concatenate([hist, st], axis=1), W2, b2, y, taps, dil)
    y_ct = _t(y).permute(0, 2, 1)
    w1, w2 = (_t(w).reshape(C, taps, C).permute(0, 2, 1).contiguous() for w in (W1, W2))
    t_o = O.causal_conv1d(F.silu(y_ct), w1, _t(b1), dilation=dil)
    want = (O.causal_conv1d(F.silu(t_o), w2, _t(b2), dilation=dil) + y_ct).permute(0, 2, 1).numpy()
    _close(v, want, "voc_conv_ref chained = one ResBlock1 step of the oracle")


@pytest.mark.parametrize("mname", ["H3", "H1"])
@pytest.mark.parametrize("C", [16, 32])
def test_voc_conv_rule_bites_on_deliberate_errors(C, mname):
    """the comparison rule of tests/test_gpu_voc_conv.py (voc_conv_cases.rule / bound_of) on reference-versus-mutated-reference, at the GPU test's
    shapes and operands as the planes hold them: a reversed tap order, a dilation off by one, a first input row off by one (both ways), the residual
    of the wrong stream and -- C = 16 -- the last odd tap counted twice each exceed the bound of the fp32 rows AND of the SiLU'd planes; the
    float32 restatement itself passes"""
    import voc_conv_cases as V
    mode, B, T = V.MODES[mname], 3, V.TILE[C]
    for m in V.group(900 + C, C, B, T, V.RES_K, V.RES_D, "c2"):
        a, alo, w, wlo = V.cpu_operands(m, mode)
        q = V.rule(m, mode, a, alo, w, wlo)
        bv, bs = V.bound_of(q["v64"], q["v32"], q["extra"], q["ceiling"]), V.bound_of(q["s64"], q["s32"], q["extra_p"], q["ceiling_p"])
        assert np.abs(q["v32"] - q["v64"]).max() <= bv and np.abs(q["s32"] - q["s64"]).max() <= bs
        taps, Cc = m["taps"], m["C"]
        w_rev = w.reshape(Cc, taps, Cc)[:, ::-1].reshape(Cc, -1)
        w_twice = w.copy()
        w_twice[:, (taps - 1) * Cc:] *= 2.0
        res = V.res_rows(m)
        mutants = {"tap order reversed": dict(w=w_rev), "dilation off by one": dict(dil=m["dil"] - 1 if m["dil"] > 1 else 2),
                   "first row one early": dict(a_row0=m["a_row0"] - 1), "first row one late": dict(a_row0=m["a_row0"] + 1),
                   "residual of the wrong stream": dict(res=np.roll(res, 1, axis=0))}
        if C == 16:
            assert taps % 2 == 1
            mutants["last odd tap counted twice"] = dict(w=w_twice)
        for what, mut in mutants.items():
            mut = dict(mut)
            v64, s64, _, _ = V.reference(m, a, mut.pop("w", w), res=mut.pop("res", None), **mut)
            assert np.abs(v64 - q["v64"]).max() > bv, (what, taps, "fp32 rows")
            assert np.abs(s64 - q["s64"]).max() > bs, (what, taps, "SiLU'd planes")


def test_ring_wrap_runs_straddle_the_capacity_on_the_oracles_trace(monkeypatch):
    """test_gpu_parity.py replays max_seq_frames = 160 / buffer_frames = 16 streams at hist_cap = 32 through every decode path.  On the oracle's own
    state machine (StreamSession; the transformer stubbed out -- positions do not depend on it) every such run has a re-prefill whose na-frame window
    straddles a multiple of 32 in the prediction ring and in the content ring, and a delay fill whose d entries do"""
    import step_ops_cases as S
    monkeypatch.setattr(O.DualAR, "slow_forward", lambda self, x, pos: (torch.zeros(768), torch.zeros(8192)))
    monkeypatch.setattr(O.DualAR, "decode_tokens", lambda self, x, pos, ns, nf, forced=None: dict(
        semantic=0, codes=torch.zeros(8, dtype=torch.int32), hidden=None, logits=None, fast_logits=None))
    W = _int_tables(np.random.default_rng(0), 768)
    kw = S.WRAP_KW
    per_prompt = {}
    for Rp in sorted(set(S.WRAP_PROMPTS)):
        sess = O.StreamSession(W, torch.zeros(Rp, dtype=torch.long), torch.zeros(8, Rp, dtype=torch.long), torch.zeros(4), torch.zeros(32, 4), noise_fn=lambda f: (None, None),
                               delay=kw["delay"], max_seq_frames=kw["max_seq_frames"], buffer_frames=kw["buffer_frames"], decode_chunk_frames=kw["chunk_frames"])
        res, ncon = [], 0
        for i in range(S.WRAP_CHUNKS):
            before = sess.n_reprefill
            sess.process_one_chunk(torch.zeros(1, 2048), content_override=torch.zeros(1, dtype=torch.long), vocode=False)
            ncon += 1
            if sess.n_reprefill != before:
                res.append((sess.frame_idx, ncon, min(kw["buffer_frames"], sess.frame_idx)))
        per_prompt[Rp] = res
        assert res and all(nf >= na >= kw["delay"] and ncon < 4096 for nf, ncon, na in res)          # (every slot of the GPU runs re-prefills)
    assert kw["buffer_frames"] + kw["delay"] + kw["chunk_frames"] < S.WRAP_CAP
    for B, _, _ in S.WRAP_RUNS:
        got = [S.wrap_straddles(per_prompt[Rp], S.WRAP_CAP, kw["delay"]) for Rp in S.WRAP_PROMPTS[:B]]
        for what in ("pred", "content", "fill"):
            assert any(g[what] for g in got), (B, what, got)
    assert all(S.wrap_straddles(per_prompt[112], S.WRAP_CAP, kw["delay"]).values())          # (slot 0 alone, the one-stream run)
