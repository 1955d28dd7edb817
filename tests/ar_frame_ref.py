"""float64 reference of ONE dual-AR decode frame from an explicit state, for the whole-frame tests of the three decode paths
(test_gpu_ar_frame.py) -- DualAR.decode_one / slow_forward / fast_decode / _block of oracle/sva_oracle.py restated in NumPy float64.

The state is what a frame reads: the slow K / V rows of positions [0, last_pos] of every layer, `cached_audio_emb` and `last_pos`.  The GPU
tests read all of it back from the engine before the frame, so a frame is judged alone: the error of the prefill and of earlier frames is in
the state, not in the frame's budget.  tests/test_ar_frame_ref_cpu.py pins frame_fp64 to the oracle's own decode_one on the oracle's own
state and measures the float32 oracle's distance from it, the constants ORACLE_K below.

Precision variants: half=True rounds the Linear weights to fp16 first, as the engine does for ar_dtype = 1 (csrc/packer.hip: weight());
norm weights and embedding tables stay float32.  The state is taken as stored (an fp16 cache was widened exactly).  The frame's own two
K / V rows enter the attention as computed, or -- kv_stored -- as the engine's fp16 cache hands them back: the persistent kernels do the
former, the multi-launch chain the latter (test_gpu_ar_frame.py says which path is held to which, and why).

RoPE uses the engine's table values (streamvoiceanon_amd.engine.rope_table: cos / sin rounded to bf16)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23

# ---- measured distance of the float32 oracle from frame_fp64 ------------------------------------------------------------------------------
# max |oracle_fp32 - frame_fp64| / (EPS32 * max |frame_fp64 quantity|), over the cases of tests/test_ar_frame_ref_cpu.py (reduced configs up to
# the last cache position, and full-size frames on weights0 -- the largest are the full-size frame at the cache end: 5.76, 8.84, 9.21, 6.91,
# 0.97), with a tenth of headroom for another host's float32 BLAS, rounded up.  That test asserts the oracle stays within these and that they
# stay within 2 x the measurement; the GPU tests
# allow the kernels 4 x as much -- they sum in other orders (split-K over waves, MFMA 4-wide, an LDS merge) -- plus 4 ulp32 of the scale:
#     |kernel - frame_fp64| <= 4 * ORACLE_K[q] * EPS32 * max |frame_fp64 q| + 4 ulp32(max |frame_fp64 q|)
# A new K / V row of an fp16 cache gets one fp16 ulp of its float64 value on top.
ORACLE_K = dict(slow_logits=7.0, fast_logits=10.0, hidden=11.0, kv=8.0, emb=1.25)
QUANTITIES = tuple(ORACLE_K)
KERNEL_FACTOR = 4.0


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bound(q, ref):
    """the GPU tests' allowance for quantity q given its float64 reference values"""
    scale = float(np.abs(ref).max())
    return KERNEL_FACTOR * ORACLE_K[q] * EPS32 * scale + 4.0 * ulp32(scale)


def ulp16(x):
    """one fp16 ulp of |x|, elementwise (fp16 cache rows)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float16)).astype(np.float64)


# ---- weights ----------------------------------------------------------------------------------------------------------------------------------
_LIN = ("attention.wqkv", "attention.wo", "feed_forward.w1", "feed_forward.w3", "feed_forward.w2")


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def build_w64(W, cfg, half=False):
    """The AR's weights for frame_fp64: Linear matrices as float64 (through fp16 when `half`), norm weights as float64, embedding tables kept
    float32 (rows are widened when gathered).  About 1 GB for the full-size model: build once per module and drop it at teardown."""
    from streamvoiceanon_amd.engine import rope_table

    def lin(name):
        a = _np(W[name])
        if half:
            a = a.astype(np.float16)
        return a.astype(np.float64)

    def vec(name):
        return _np(W[name]).astype(np.float64)

    m = "arvc.decoder.model."

    def layer(p):
        d = {k.split(".")[1]: lin(p + k + ".weight") for k in _LIN}
        d["attn_norm"], d["ffn_norm"] = vec(p + "attention_norm.weight"), vec(p + "ffn_norm.weight")
        return d

    hd = cfg.dim // cfg.n_head
    return dict(cfg=cfg, half=bool(half), hd=hd,
                slow=[layer(m + f"layers.{l}.") for l in range(cfg.n_layer)],
                fast=[layer(m + f"fast_layers.{l}.") for l in range(cfg.n_fast_layer)],
                out_w=lin(m + "output.weight"), out_norm=vec(m + "norm.weight"),
                fast_out_w=lin(m + "fast_output.weight"), fast_norm=vec(m + "fast_norm.weight"),
                content_emb=_np(W["arvc.embedding.weight"]), codebook_emb=_np(W[m + "codebook_embeddings.weight"]),
                fast_emb=_np(W[m + "fast_embeddings.weight"]),
                rope=rope_table(cfg.max_seq_len, hd).astype(np.float64), rope_fast=rope_table(cfg.num_codebooks, hd).astype(np.float64))


# ---- the transformer block -----------------------------------------------------------------------------------------------------------------
def _rms(x, w, eps=1e-5):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def _rope(x, tab):
    """x [M, H, hd], tab [M, hd/2, 2]: adjacent pairs (x0, x1) -> (x0 c - x1 s, x1 c + x0 s)"""
    xs = x.reshape(x.shape[0], x.shape[1], -1, 2)
    c, s = tab[:, None, :, 0], tab[:, None, :, 1]
    return np.stack([xs[..., 0] * c - xs[..., 1] * s, xs[..., 1] * c + xs[..., 0] * s], axis=-1).reshape(x.shape)


def _block(x, L, tab, kc, vc, pos, H, hd, stored=None):
    """TransformerBlock on rows x [M, dim] at positions pos [M]; kc / vc [H, n, hd] hold the rows below pos[0] and receive the new ones, or
    `stored` = (k, v) [M, H, hd] in their place.  Returns (x_out, k_new [M, H, hd], v_new [M, H, hd]) as computed."""
    M = x.shape[0]
    qkv = _rms(x, L["attn_norm"]) @ L["wqkv"].T
    q, k, v = np.split(qkv, 3, axis=-1)
    q = _rope(q.reshape(M, H, hd), tab[pos])
    k = _rope(k.reshape(M, H, hd), tab[pos])
    v = v.reshape(M, H, hd)
    if stored is not None:                                         # (k, v) [M, H, hd] as the engine's cache holds them after the frame
        kc[:, pos], vc[:, pos] = stored[0].transpose(1, 0, 2), stored[1].transpose(1, 0, 2)
    else:
        kc[:, pos], vc[:, pos] = k.transpose(1, 0, 2), v.transpose(1, 0, 2)
    y = np.empty((M, H, hd))
    for m in range(M):
        n = int(pos[m]) + 1                                        # causal: keys 0 .. pos[m]
        sc = np.einsum("hd,hld->hl", q[m], kc[:, :n]) / np.sqrt(hd)
        sc = np.exp(sc - sc.max(-1, keepdims=True))
        y[m] = np.einsum("hl,hld->hd", sc / sc.sum(-1, keepdims=True), vc[:, :n])
    x = x + y.reshape(M, H * hd) @ L["wo"].T
    h = _rms(x, L["ffn_norm"])
    g = h @ L["w1"].T
    return x + ((g / (1.0 + np.exp(-g))) * (h @ L["w3"].T)) @ L["w2"].T, k, v


# ---- one frame ---------------------------------------------------------------------------------------------------------------------------------
def frame_fp64(W64, state, content_code, forced, noise=None, sampling=(0.7, 0.7), kv_stored=None):
    """DualAR.decode_one, teacher-forced.  state: dict(k, v: [n_layer, H, >= last_pos + 1, hd] (rows [0, last_pos] are read), emb: [dim]
    (cached_audio_emb), last_pos).  forced int [num_codebooks]: the codes fed to the fast AR and embedded for the next frame.
    noise (optional) = (slow [vocab], fast [num_codebooks, codebook_size]) Exp(1) draws: then `codes` / `semantic` are the oracle's
    sample_token evaluated in float64 on the reference logits with the pair `sampling` = (temperature, top_p).
    kv_stored = (k, v) [n_layer, 2, H, hd]: the attention reads these rows -- the ones the engine's fp16 cache
    holds after the frame -- in place of its own.  Rounding to fp16 is a step function: a float32 value that sits within its own rounding error
    of an fp16 tie stores one whole fp16 ulp away from the float64 value's rounding, which no float32-sized bound downstream can absorb.  The
    stored rows are still compared with k_new / v_new (to one fp16 ulp); what follows them is compared given them.

    Returns dict: slow_logits [vocab], fast_logits [num_codebooks, codebook_size], hidden [dim] (pre-norm, content row), k_new / v_new
    [n_layer, 2, H, hd] (the rows of positions last_pos + 1, + 2), emb [dim] (the new cached_audio_emb), last_pos (+ 2); and, for the error-scale
    bookkeeping of the CPU test, x_layers [n_layer, 2, dim] (the rows entering each slow layer) and fast_hidden [num_codebooks, dim]."""
    cfg, hd = W64["cfg"], W64["hd"]
    H, ncb, cbs = cfg.n_head, cfg.num_codebooks, cfg.codebook_size
    lp = int(state["last_pos"])
    pos = np.array([lp + 1, lp + 2])
    assert lp >= 0 and lp + 2 < cfg.max_seq_len, "the frame's rows must fit the cache"
    forced = np.asarray(forced).astype(np.int64).reshape(ncb)
    x = np.stack([np.asarray(state["emb"], np.float64), W64["content_emb"][int(content_code)].astype(np.float64)])
    k_new, v_new = np.empty((cfg.n_layer, 2, H, hd)), np.empty((cfg.n_layer, 2, H, hd))
    x_layers = np.empty((cfg.n_layer, 2, cfg.dim))                  # the two rows entering each slow layer (for error-scale bookkeeping)
    for l in range(cfg.n_layer):
        x_layers[l] = x
        kc, vc = np.empty((H, lp + 3, hd)), np.empty((H, lp + 3, hd))
        kc[:, :lp + 1], vc[:, :lp + 1] = state["k"][l][:, :lp + 1], state["v"][l][:, :lp + 1]
        x, k_new[l], v_new[l] = _block(x, W64["slow"][l], W64["rope"], kc, vc, pos, H, hd,
                                       None if kv_stored is None else (kv_stored[0][l], kv_stored[1][l]))
    hidden = x[-1]
    slow_logits = _rms(hidden, W64["out_norm"]) @ W64["out_w"].T
    # fast AR: 8 steps over its own cache of at most 8 positions, cleared every frame
    kf = np.zeros((cfg.n_fast_layer, H, ncb, hd))
    vf = np.zeros_like(kf)
    fast_logits, fast_hidden = np.empty((ncb, cbs)), np.empty((ncb, cfg.dim))
    xin = hidden
    for cb in range(ncb):
        h = xin[None]
        for l in range(cfg.n_fast_layer):
            h, _, _ = _block(h, W64["fast"][l], W64["rope_fast"], kf[l], vf[l], np.array([cb]), H, hd)
        fast_hidden[cb] = h[0]
        fast_logits[cb] = _rms(h[0], W64["fast_norm"]) @ W64["fast_out_w"].T
        xin = W64["fast_emb"][forced[cb]].astype(np.float64)
    emb = W64["codebook_emb"][forced + np.arange(ncb) * cbs].astype(np.float64).sum(0)
    out = dict(slow_logits=slow_logits, fast_logits=fast_logits, hidden=hidden, k_new=k_new, v_new=v_new, emb=emb, last_pos=lp + 2,
               x_layers=x_layers, fast_hidden=fast_hidden)
    if noise is not None:
        out["semantic"] = sample_f64(slow_logits, noise[0], *sampling)[0]
        out["codes"] = np.array([sample_f64(fast_logits[cb], noise[1][cb], *sampling)[0] for cb in range(ncb)], np.int32)
    return out


# ---- the oracle's sampler in float64, with its distance from a tie ----------------------------------------------------------------------------
TIE = 1e-5


def sample_f64(logits, noise, temperature, top_p):
    """(token, near_tie): O.sample_token on float64 tensors.  near_tie = the only cases in which a float32 sampler on the same logits may
    legitimately pick another token: the winner's ratio p / noise leads the runner-up by less than TIE relative, or the sorted inclusive
    cumulative softmax passes top_p within TIE relative of it (the nucleus boundary) AND the token at that boundary wins when it is kept --
    keeping or dropping any other token only rescales every ratio alike."""
    import torch
    from oracle import sva_oracle as O

    l64 = np.asarray(logits, np.float64)
    n64 = np.asarray(noise, np.float64)
    p = O.token_probs(torch.from_numpy(l64.copy()), temperature, top_p)
    r = p.numpy() / n64
    tok = int(r.argmax())
    top2 = np.partition(r, -2)[-2:]
    near = bool(top2[1] - top2[0] <= TIE * top2[1])
    order = np.argsort(-l64, kind="stable")
    s = l64[order]
    if top_p > 0:
        e = np.exp(s - s[0])
        cum = np.cumsum(e / e.sum())
        i = int(np.abs(cum - top_p).argmin())
        if i > 0 and abs(cum[i] - top_p) <= TIE * top_p:           # token `order[i]` is in or out by a rounding: does it win when in?
            score = s[:i + 1] / max(temperature, 1e-5) - np.log(n64[order[:i + 1]])
            near = near or bool(score[i] >= score[:i].max() - TIE)
    else:                                                           # greedy: only rank 0 survives; a tie is two equal top logits
        near = near or bool(s[0] - s[1] <= TIE * max(abs(s[0]), 1.0))
    return tok, near


# ---- positions ---------------------------------------------------------------------------------------------------------------------------------
def last_pos_after_fill(R_frames, delay, nspk=33):
    """last_pos of a stream at its first decoded frame: prefill_prompt writes the speaker prefix and 2 R rows (rows 0 .. nspk + 2 R - 1),
    prefill_src_condition4delay 2 delay - 1 more.  test_ar_frame_ref_cpu.py holds the oracle's DualAR to this."""
    return nspk + 2 * R_frames - 1 + 2 * delay - 1


def long_prompt_frames(max_seq_len, delay, nspk=33):
    """the prompt length whose first decoded frame starts at last_pos = max_seq_len - 33: its 16th frame writes the last two cache rows"""
    R_frames, rem = divmod(max_seq_len - 33 - (nspk - 1 + 2 * delay - 1), 2)
    assert rem == 0 and (max_seq_len - 1 - last_pos_after_fill(R_frames, delay, nspk)) == 32
    return R_frames


# ---- states ---------------------------------------------------------------------------------------------------------------------------------------
def state_from_oracle(ar):
    """the oracle's own cache and embedding as a state (DualAR after prefill_src_condition4delay / decode_one)"""
    n = ar.last_pos + 1
    return dict(k=ar.k[:, :, :n].numpy().astype(np.float64), v=ar.v[:, :, :n].numpy().astype(np.float64),
                emb=ar.cached_new_audio_emb[0].numpy().astype(np.float64), last_pos=int(ar.last_pos))


def state_from_batch(b, slot, last_pos, emb_row):
    """the engine's: Batch.kv_rows over [0, last_pos] -> k, v [layers, H, n, 64], and the slot's row of the "cached_audio_emb" tap"""
    kv = b.kv_rows(slot, 0, last_pos + 1)
    return dict(k=kv[:, 0], v=kv[:, 1], emb=np.asarray(emb_row, np.float64), last_pos=int(last_pos))
