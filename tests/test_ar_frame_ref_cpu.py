"""tests/ar_frame_ref.py pinned to the oracle on the CPU: frame_fp64 fed the oracle's OWN cache rows and embedding reproduces the float32
oracle's decode_one -- logits, hidden, the new cache rows, the new embedding -- to the oracle's rounding.

Two bounds, neither picked:
  * a priori: |oracle - frame_fp64| <= n_stage * EPS32 * sum |w| |x| of the quantity's last linear map, evaluated on the reference's own
    operands (n_stage = the Linear maps in front of the quantity: every one of them rounds like one float32 dot product of that size);
  * measured: the same distance in units of EPS32 * max |reference| is the table ORACLE_K of ar_frame_ref.py, from which the GPU tests derive
    what they allow the kernels.  The table must cover the measurement and must not exceed 2 x it.
Cases: reduced models (dim 128, 4 heads of 32, 2 + 2 layers) through prefill, delay fill and 3 teacher-forced frames, one of them ending
on max_seq_len - 1; the full-size model on weights0 for one frame after a 3-frame prompt, and for one frame at the last two positions of the
2048-row cache over a planted state."""
import dataclasses

import numpy as np
import pytest
import torch

import ar_frame_ref as R

torch.set_grad_enabled(False)

_MEASURED = {}
_TIES = [0, 0]           # (sampled codes within TIE of a tie, sampled codes) over the oracle's frames of this file


def _reduced(max_seq_len, seed):
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import specs

    mc = dataclasses.replace(specs.ModelConfig(), ar_dim=128, ar_heads=4, ar_layers=2, ar_fast_layers=2, ar_inter=256, ar_vocab=512, codebook_size=64,
                             max_seq_len=max_seq_len)
    cfg = O.ARConfig(dim=128, n_head=4, n_layer=2, n_fast_layer=2, inter=256, vocab=512, codebook_size=64, num_codebooks=8, max_seq_len=max_seq_len)
    return O.load_synth_weights(seed, specs.arvc_specs(mc)), cfg


def _noise(rng, cfg):
    return (rng.exponential(size=cfg.vocab).astype(np.float32) + 1e-9, rng.exponential(size=(cfg.num_codebooks, cfg.codebook_size)).astype(np.float32) + 1e-9)


def _sabs(W64, st, code, forced):
    """(reference frame, sum |w| |x| of the last linear map in front of every quantity, on the reference's own operands)"""
    cfg, H, hd = W64["cfg"], W64["cfg"].n_head, W64["hd"]
    out = R.frame_fp64(W64, st, code, forced)
    ab = np.abs
    s = {}
    s["slow_logits"] = ab(R._rms(out["hidden"], W64["out_norm"])) @ ab(W64["out_w"]).T
    s["fast_logits"] = ab(R._rms(out["fast_hidden"], W64["fast_norm"])) @ ab(W64["fast_out_w"]).T
    # hidden = the residual stream after the last layer's w2: |x| + |w2| |act| with the layer's own FFN operands (x ~ hidden in front of w2)
    L = W64["slow"][-1]
    h = R._rms(out["hidden"], L["ffn_norm"])
    g = h @ L["w1"].T
    s["hidden"] = ab(out["hidden"]) + ab((g / (1.0 + np.exp(-g))) * (h @ L["w3"].T)) @ ab(L["w2"]).T
    # new rows of layer l: |wqkv_l| |rmsnorm(x_l)|; RoPE mixes the two elements of a pair: both get the pair's sum
    s["kv"] = np.empty(out["k_new"].shape)
    for l in range(cfg.n_layer):
        qkv = ab(R._rms(out["x_layers"][l], W64["slow"][l]["attn_norm"])) @ ab(W64["slow"][l]["wqkv"]).T
        k = qkv[:, cfg.dim:2 * cfg.dim].reshape(2, H, hd // 2, 2).sum(-1, keepdims=True).repeat(2, -1).reshape(2, H, hd)
        s["kv"][l] = np.maximum(k, qkv[:, 2 * cfg.dim:].reshape(2, H, hd))
    s["emb"] = ab(W64["codebook_emb"][np.asarray(forced, np.int64) + np.arange(cfg.num_codebooks) * cfg.codebook_size].astype(np.float64)).sum(0)
    return out, s


def _compare(tag, W64, st, code, forced, aux, ar_after):
    """one oracle frame against frame_fp64 on the state it started from; records the measured distances"""
    cfg = W64["cfg"]
    ref, sabs = _sabs(W64, st, code, forced)
    lp = st["last_pos"]
    got = dict(slow_logits=aux["logits"].numpy().astype(np.float64), fast_logits=aux["fast_logits"].numpy().astype(np.float64),
               hidden=aux["hidden"].numpy().astype(np.float64), emb=ar_after.cached_new_audio_emb[0].numpy().astype(np.float64))
    kn = ar_after.k[:, :, lp + 1:lp + 3].numpy().astype(np.float64).transpose(0, 2, 1, 3)          # [L, 2, H, hd]
    vn = ar_after.v[:, :, lp + 1:lp + 3].numpy().astype(np.float64).transpose(0, 2, 1, 3)
    # (the embedding is a float32 sum of num_codebooks table rows: num_codebooks - 1 additions of half an EPS32 each)
    n_stage = dict(slow_logits=5 * cfg.n_layer + 1, hidden=5 * cfg.n_layer, kv=5 * cfg.n_layer, emb=(cfg.num_codebooks - 1) / 2,
                   fast_logits=5 * (cfg.n_layer + cfg.n_fast_layer) + 2)
    assert ref["last_pos"] == ar_after.last_pos == lp + 2
    for q in R.QUANTITIES:
        if q == "kv":
            err = np.maximum(np.abs(kn - ref["k_new"]), np.abs(vn - ref["v_new"]))
            scale = max(np.abs(ref["k_new"]).max(), np.abs(ref["v_new"]).max())
        else:
            err = np.abs(got[q] - ref[q])
            scale = np.abs(ref[q]).max()
        lim = n_stage[q] * R.EPS32 * sabs[q]
        assert (err <= lim).all(), (tag, q, float(err.max()), float((err / lim).max()))
        k = float(err.max() / (R.EPS32 * scale))
        _MEASURED.setdefault(q, {})[tag] = k
    # the state below the new rows is what went in
    np.testing.assert_array_equal(ar_after.k[:, :, :lp + 1].numpy(), st["k"].astype(np.float32))
    return ref


def _run_reduced(R_frames, max_seq_len, seed, end_on_last):
    from oracle import sva_oracle as O
    from streamvoiceanon_amd.synth_audio import synth_prompt

    W, cfg = _reduced(max_seq_len, seed)
    W64 = R.build_w64(W, cfg)
    ac, cc, style, timbre = synth_prompt(4000 + seed, R_frames, codebook_size=cfg.codebook_size, vocab=cfg.vocab)
    ar = O.DualAR(W, cfg)
    ar.prefill_prompt(torch.from_numpy(cc), torch.from_numpy(ac), torch.from_numpy(style), torch.from_numpy(timbre), 2)
    rng = np.random.default_rng(seed)
    ar.prefill_src_condition4delay(torch.from_numpy(rng.integers(0, cfg.vocab, 2)))
    assert ar.last_pos == R.last_pos_after_fill(R_frames, 2, cfg.n_spk_tokens)
    near = total = 0
    for f in range(3):
        st = R.state_from_oracle(ar)
        code = int(rng.integers(0, cfg.vocab))
        forced = rng.integers(0, cfg.codebook_size, cfg.num_codebooks).astype(np.int32)
        ns, nf = _noise(rng, cfg)
        codes, last, aux = ar.decode_one(code, torch.from_numpy(ns), torch.from_numpy(nf), forced=torch.from_numpy(forced))
        ref = _compare(f"reduced S={max_seq_len} R={R_frames} frame {f}", W64, st, code, forced, aux, ar)
        # the oracle's own sampled codes against its sampler in float64 on ITS logits: equal unless within TIE of a tie
        for cb in range(cfg.num_codebooks):
            tok, nt = R.sample_f64(aux["fast_logits"][cb].numpy(), nf[cb], 0.7, 0.7)
            total += 1
            near += int(nt)
            assert nt or tok == int(codes[cb]), (f, cb)
        del ref
    if end_on_last:
        assert ar.last_pos == max_seq_len - 1
    _TIES[0] += near
    _TIES[1] += total


@pytest.mark.parametrize("R_frames,max_seq_len,seed,end_on_last", [(3, 64, 0, False), (11, 64, 1, True), (100, 256, 2, False)])
def test_frame_fp64_equals_the_oracle_on_reduced_models(R_frames, max_seq_len, seed, end_on_last):
    _run_reduced(R_frames, max_seq_len, seed, end_on_last)


@pytest.fixture(scope="module")
def w64_full(weights0):
    from oracle import sva_oracle as O
    W64 = R.build_w64(weights0, O.ARConfig())
    yield W64
    W64.clear()


def test_frame_fp64_equals_the_oracle_full_size_one_frame(weights0, w64_full):
    from oracle import sva_oracle as O
    from streamvoiceanon_amd.synth_audio import frame_noise, synth_prompt

    cfg = O.ARConfig()
    ac, cc, style, timbre = synth_prompt(7001, 3)
    ar = O.DualAR(weights0, cfg)
    ar.prefill_prompt(torch.from_numpy(cc), torch.from_numpy(ac), torch.from_numpy(style), torch.from_numpy(timbre), 2)
    ar.prefill_src_condition4delay(torch.tensor([17, 4242]))
    assert ar.last_pos == 32 + 2 * 3 + 3 == R.last_pos_after_fill(3, 2, cfg.n_spk_tokens)
    assert R.long_prompt_frames(cfg.max_seq_len, 2, cfg.n_spk_tokens) == 990
    st = R.state_from_oracle(ar)
    forced = np.array([3, 999, 0, 512, 77, 250, 801, 640], np.int32)
    ns, nf = frame_noise(7001, 0)
    codes, _, aux = ar.decode_one(8191, torch.from_numpy(ns), torch.from_numpy(nf), forced=torch.from_numpy(forced))
    _compare("full R=3 frame 0", w64_full, st, 8191, forced, aux, ar)
    near = 0
    for cb in range(8):
        tok, nt = R.sample_f64(aux["fast_logits"][cb].numpy(), nf[cb], 0.7, 0.7)
        near += int(nt)
        assert nt or tok == int(codes[cb]), cb
    _TIES[0] += near
    _TIES[1] += 8


def test_frame_fp64_equals_the_oracle_full_size_at_the_cache_end(weights0, w64_full):
    """the frame whose rows are max_seq_len - 2 and max_seq_len - 1 over a planted state of 2046 rows (a prefill of that length on the CPU
    would take minutes; the frame's arithmetic does not care where its state came from)"""
    from oracle import sva_oracle as O
    from streamvoiceanon_amd.synth_audio import frame_noise

    cfg = O.ARConfig()
    ar = O.DualAR(weights0, cfg)
    g = torch.Generator().manual_seed(5)
    n = cfg.max_seq_len - 2
    ar.k[:, :, :n] = torch.randn(cfg.n_layer, cfg.n_head, n, 64, generator=g) * 0.8
    ar.v[:, :, :n] = torch.randn(cfg.n_layer, cfg.n_head, n, 64, generator=g) * 0.8
    ar.last_pos, ar.delay = n - 1, 2
    ar.cached_new_audio_emb = ar.embed_audio(torch.tensor([5, 6, 7, 8, 9, 10, 11, 12])[:, None])
    st = R.state_from_oracle(ar)
    forced = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.int32)
    ns, nf = frame_noise(7002, 0)
    _, last, aux = ar.decode_one(1234, torch.from_numpy(ns), torch.from_numpy(nf), forced=torch.from_numpy(forced))
    assert last == cfg.max_seq_len - 1
    _compare("full planted frame at S-2, S-1", w64_full, st, 1234, forced, aux, ar)


def test_oracle_k_table_is_the_measurement(record_property):
    """runs last in this file: ORACLE_K covers every measured distance and is at most 2 x the largest"""
    assert len(_MEASURED) == len(R.QUANTITIES) and all(len(v) >= 11 for v in _MEASURED.values()), "the measuring tests above did not all run"
    for q in R.QUANTITIES:
        worst_tag = max(_MEASURED[q], key=_MEASURED[q].get)
        worst = _MEASURED[q][worst_tag]
        print(f"[ar frame ref] {q}: oracle fp32 distance {worst:.3f} x EPS32 x max|ref| ({worst_tag}); table {R.ORACLE_K[q]}")
        record_property(f"oracle_k_{q}", dict(measured=worst, case=worst_tag, table=R.ORACLE_K[q]))
    for q in R.QUANTITIES:
        worst = max(_MEASURED[q].values())
        assert worst <= R.ORACLE_K[q] <= 2.0 * worst, (q, worst, R.ORACLE_K[q])
    # the float32 oracle alone stays within the cap on near-ties that the GPU test allows itself (1 % of the sampled codes)
    assert _TIES[1] >= 80 and _TIES[0] <= 0.01 * _TIES[1], _TIES
