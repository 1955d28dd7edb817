"""NumPy restatements of the non-GEMM operations, written from their definitions (csrc/kernels.h, oracle/sva_oracle.py), for the
per-kernel GPU tests (test_gpu_kernels.py), and of the conv-GEMM with its prologues and epilogues (csrc/sva_common.h: ConvGemm) for
test_gpu_conv_gemm.py.  tests/test_kernel_refs.py pins each of them to the oracle's own function (the conv-GEMM: to torch's conv1d) on the CPU.

Every function takes `dt`: np.float64 is THE reference; np.float32 evaluates the same formula naively in float32 (sequential sums,
float32 exp / tanh / sqrt), which gives the per-case rounding scale e32 = max |f32 - f64| the GPU tests derive their bounds from
(`bound`).  Layouts are the kernels' (channel-last rows); RoPE is the engine's: adjacent pairs, table rounded to bf16."""
import numpy as np

N_FFT, HOP = 2048, 512


# ---- arithmetic helpers ------------------------------------------------------------------------------------------------------------
def _sum(x, dt):
    """sum over the last axis; float32: strictly sequential (cumsum), float64: numpy's pairwise sum"""
    x = np.asarray(x, dt)
    return np.cumsum(x, axis=-1, dtype=dt)[..., -1] if dt == np.float32 else x.sum(-1)


def _matmul(a, b, dt):
    """a [..., M, K] @ b [..., K, N]; float32: one rank-1 update per k in ascending order (the naive sequential dot product)"""
    a, b = np.asarray(a, dt), np.asarray(b, dt)
    if dt != np.float32:
        return a @ b
    acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), dt)
    for k in range(a.shape[-1]):
        acc += a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return acc


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def e32_of(f32ref, f64ref):
    """max |f32ref - f64ref|: the rounding scale of the naive float32 evaluation"""
    return float(np.abs(np.asarray(f32ref, np.float64) - np.asarray(f64ref, np.float64)).max()) if np.size(f64ref) else 0.0


def bound(e32, f64ref, extra=0.0):
    """4 e32 + 4 ulp32(max |ref|) (+ a derived, documented extra term)"""
    return 4.0 * e32 + 4.0 * ulp32(np.abs(np.asarray(f64ref, np.float64)).max() if np.size(f64ref) else 0.0) + extra


def round_f16(x):
    """values as an fp16 cache / plane holds them"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


# ---- RoPE ----------------------------------------------------------------------------------------------------------------------------
def rope_table(n_pos, hd=64):
    """[n_pos, hd/2, 2] (cos, sin), rounded to bf16 -- the engine's table (oracle.sva_oracle.rope_table)"""
    from oracle import sva_oracle as O
    return O.rope_table(n_pos, hd).numpy().astype(np.float64)


def apply_rope(x, tab, dt=np.float64):
    """x [..., hd] rotated by tab [..., hd/2, 2] (broadcast over the leading axes): adjacent pairs (x0, x1) -> (x0 c - x1 s, x1 c + x0 s)"""
    x = np.asarray(x, dt)
    c, s = np.asarray(tab[..., 0], dt), np.asarray(tab[..., 1], dt)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = x0 * c - x1 * s
    out[..., 1::2] = x1 * c + x0 * s
    return out


# ---- row operations ---------------------------------------------------------------------------------------------------------------
def rms_norm(x, w, eps, dt=np.float64):
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    ms = _sum(x * x, dt) / dt(x.shape[-1])
    return x * (dt(1) / np.sqrt(ms + dt(eps)))[..., None] * w


def layer_norm(x, w, b, eps, dt=np.float64):
    """biased variance over the last axis"""
    x, w, b = np.asarray(x, dt), np.asarray(w, dt), np.asarray(b, dt)
    mean = (_sum(x, dt) / dt(x.shape[-1]))[..., None]
    d = x - mean
    var = (_sum(d * d, dt) / dt(x.shape[-1]))[..., None]
    return d * (dt(1) / np.sqrt(var + dt(eps))) * w + b


def dwconv7_ln(x, wT, bias, ln_w, ln_b, eps, dt=np.float64):
    """x [B, T + 6, C] (6 history rows first), wT [7, C] tap-major: y[t] = bias + sum_j wT[j] x[t + j], then LayerNorm over C"""
    x, wT = np.asarray(x, dt), np.asarray(wT, dt)
    T = x.shape[1] - 6
    y = np.broadcast_to(np.asarray(bias, dt), (x.shape[0], T, x.shape[2])).copy()
    for j in range(7):
        y += wT[j] * x[:, j:j + T]
    return layer_norm(y, ln_w, ln_b, eps, dt)


def bsq(z, norm_w, eps, W, bias, dt=np.float64):
    """rows z [R, C] -> (zn [R, C] (= z without norm_w), u [R, nbits] L2-normalised, raw projection [R, nbits], index int64 [R] MSB first)"""
    zn = rms_norm(z, norm_w, eps, dt) if norm_w is not None else np.asarray(z, dt)
    raw = _matmul(zn, np.asarray(W, dt).T, dt) + np.asarray(bias, dt)
    nrm = np.sqrt(_sum(raw * raw, dt))
    u = raw / np.maximum(nrm, dt(1e-12))[..., None]
    nbits = raw.shape[-1]
    idx = ((raw > 0).astype(np.int64) << np.arange(nbits - 1, -1, -1, dtype=np.int64)).sum(-1)
    return zn, u, raw, idx


FSQ_LEVELS = np.array([8, 5, 5, 5])
FSQ_BASIS = np.array([1, 8, 40, 200])


def fsq_encode(x, Win, bin_, dt=np.float64):
    """x [B, T, G * gd], Win [G, 4, gd], bin_ [G, 4] -> (codes int32 [B, G, T], margin [B, G, T] = distance of the bounded value to the
    nearest rounding boundary).  bounded = tanh(z + shift) * half_l - offset, half_l = (L - 1)(1 + 1e-3) / 2, offset = 0.5 for even L"""
    x = np.asarray(x, dt)
    G, _, gd = Win.shape
    half_l = ((FSQ_LEVELS - 1) * (1 + 1e-3) / 2).astype(dt)
    offset = np.where(FSQ_LEVELS % 2 == 0, 0.5, 0.0).astype(dt)
    shift = np.arctanh(offset / half_l).astype(dt)
    codes, margin = [], []
    for g in range(G):
        z = _matmul(x[..., g * gd:(g + 1) * gd], np.asarray(Win[g], dt).T, dt) + np.asarray(bin_[g], dt)
        bd = np.tanh(z + shift) * half_l - offset
        q = np.rint(bd)
        codes.append(((q.astype(np.int64) + FSQ_LEVELS // 2) * FSQ_BASIS).sum(-1).astype(np.int32))
        margin.append((0.5 - np.abs(bd - q)).min(-1))
    return np.stack(codes, 1), np.stack(margin, 1)


def fsq_decode(codes, Wout, bout, dt=np.float64):
    """codes int [B, G, T], Wout [G, gd, 4], bout [G, gd] -> [B, T, G * gd]"""
    codes = np.asarray(codes, np.int64)
    outs = []
    for g in range(codes.shape[1]):
        digits = (codes[:, g, :, None] // FSQ_BASIS) % FSQ_LEVELS
        c = ((digits - FSQ_LEVELS // 2) / (FSQ_LEVELS // 2)).astype(dt)
        outs.append(_matmul(c, np.asarray(Wout[g], dt).T, dt) + np.asarray(bout[g], dt))
    return np.concatenate(outs, -1)


def conv_post_tanh(x, w, bias, dt=np.float64):
    """x [B, T + k - 1, C], w [k, C]: pcm[t] = tanh(bias + sum_j sum_c w[j, c] silu(x[t + j, c]))"""
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    k = w.shape[0]
    T = x.shape[1] - k + 1
    s = x / (dt(1) + np.exp(-x))
    cols = np.concatenate([s[:, j:j + T] for j in range(k)], -1)            # [B, T, k * C], taps outer, channels inner
    return np.tanh(_sum(cols * w.reshape(-1), dt) + dt(np.asarray(bias).reshape(-1)[0]))


# ---- STFT ---------------------------------------------------------------------------------------------------------------------------
_DFT = {}


def _dft(dt):
    if dt not in _DFT:
        n = np.arange(N_FFT, dtype=np.float64)
        ang = np.remainder(np.outer(n, np.arange(N_FFT // 2 + 1)), N_FFT) * (2.0 * np.pi / N_FFT)
        hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)                 # periodic Hann
        _DFT[dt] = (np.cos(ang).astype(dt), (-np.sin(ang)).astype(dt), hann.astype(dt))
    return _DFT[dt]


def stft_mag(window, frames=None, dt=np.float64):
    """window [B, N] in time order (oldest sample first) -> [B, n_frames, 1025]: frame m = samples [512 m - 1536, 512 m + 512) with zeros
    before the window, periodic Hann, 2048-point DFT, sqrt(re^2 + im^2 + 1e-6) (a silent frame gives 1e-3)"""
    window = np.asarray(window, dt)
    B, N = window.shape
    frames = range(N // HOP) if frames is None else frames
    cos, msin, hann = _dft(dt)
    y = np.concatenate([np.zeros((B, N_FFT - HOP), dt), window], 1)
    fr = np.stack([y[:, HOP * m:HOP * m + N_FFT] for m in frames], 1) * hann        # [B, F, 2048]
    if dt == np.float32:       # naive float32 DFT, sums in ascending sample order
        re, im = _matmul(fr, cos, dt), _matmul(fr, msin, dt)
    else:
        re, im = fr @ cos, fr @ msin
    return np.sqrt(re * re + im * im + dt(1e-6))


def ring_to_window(ring, origin):
    """ring [B, N] with the oldest sample at `origin` -> time order"""
    return np.roll(ring, -int(origin), axis=1)


# ---- attention -------------------------------------------------------------------------------------------------------------------
def _softmax_pv(s, v, dt):
    """s [L] scores (already scaled), v [L, hd] -> softmax(s) v (float32: keys accumulated in ascending order)"""
    p = np.exp(s - s.max())
    pv = np.cumsum(p[:, None] * v, axis=0, dtype=dt)[-1] if dt == np.float32 else p @ v
    return pv / _sum(p, dt)


def decode_attention(q, cache, slot, pos, H, dt=np.float64):
    """q [M, H * 64] (RoPE already applied); cache [n_slots, 2, H, S, 64] as the device holds it (fp16 caches: values already rounded);
    row m attends keys 0 .. pos[m] of slot[m]: softmax(q K^T / 8) V"""
    M = q.shape[0]
    out = np.empty((M, H * 64), dt)
    for m in range(M):
        L = int(pos[m]) + 1
        for h in range(H):
            k = np.asarray(cache[slot[m], 0, h, :L], dt)
            v = np.asarray(cache[slot[m], 1, h, :L], dt)
            s = _sum(k * np.asarray(q[m, h * 64:(h + 1) * 64], dt), dt) * dt(0.125)
            out[m, h * 64:(h + 1) * 64] = _softmax_pv(s, v, dt)
    return out


def rope_kvwrite(qkv, cache, slot, pos, tab, H, half_kv=False, dt=np.float64):
    """qkv [M, 3 D]: RoPE(pos[m]) on q and k; k, v written to cache[slot[m], :, :, pos[m]] (rounded to fp16 when half_kv).
    Returns (qkv with q rotated -- k, v columns as given --, the whole cache after the writes)"""
    qkv = np.asarray(qkv, dt)
    M, D = qkv.shape[0], H * 64
    out_q, cache = qkv.copy(), np.array(cache, dt)
    for m in range(M):
        t = tab[int(pos[m])]
        out_q[m, :D] = apply_rope(qkv[m, :D].reshape(H, 64), t, dt).reshape(D)
        k = apply_rope(qkv[m, D:2 * D].reshape(H, 64), t, dt)
        v = qkv[m, 2 * D:].reshape(H, 64)
        cache[slot[m], 0, :, int(pos[m])] = round_f16(k) if half_kv else k
        cache[slot[m], 1, :, int(pos[m])] = round_f16(v) if half_kv else v
    return out_q, cache


def enc_attention(qkv, tab, H, window=512, dt=np.float64):
    """qkv [B, T, 3 D], tab [T, 32, 2]: RoPE on q and k, causal softmax(q k^T / 8) v over keys max(0, r - window + 1) .. r -> [B, T, D]"""
    qkv = np.asarray(qkv, dt)
    B, T, D = qkv.shape[0], qkv.shape[1], H * 64
    q = apply_rope(qkv[..., :D].reshape(B, T, H, 64), tab[:T, None], dt).transpose(0, 2, 1, 3)          # [B, H, T, 64]
    k = apply_rope(qkv[..., D:2 * D].reshape(B, T, H, 64), tab[:T, None], dt).transpose(0, 2, 1, 3)
    v = qkv[..., 2 * D:].reshape(B, T, H, 64).transpose(0, 2, 1, 3)
    s = _matmul(q, k.transpose(0, 1, 3, 2), dt) * dt(0.125)
    r = np.arange(T)
    keep = (r[None, :] <= r[:, None]) & (r[None, :] > r[:, None] - window)
    s = np.where(keep, s, dt(-np.inf))
    p = np.exp(s - s.max(-1, keepdims=True))
    if dt == np.float32:
        l = np.cumsum(p, axis=-1, dtype=dt)[..., -1]
    else:
        l = p.sum(-1)
    o = _matmul(p, v, dt) / l[..., None]
    return o.transpose(0, 2, 1, 3).reshape(B, T, D)


# ---- conv-GEMM (csrc/sva_common.h: ConvGemm; epilogue order of gemm.hip) -------------------------------------------------------------
LOG_CLAMP = np.float32(1e-5)


def silu(x, dt=np.float64):
    x = np.asarray(x, dt)
    with np.errstate(over="ignore"):        # exp(-x) = inf for a very negative x: x / inf = -0, the limit
        return x / (dt(1) + np.exp(-x))


def gelu_erf(x, dt=np.float64):
    import torch
    x = np.asarray(x, dt)
    return dt(0.5) * x * (dt(1) + torch.erf(torch.from_numpy(np.ascontiguousarray(x * dt(0.70710678118654752))).clone()).numpy())


def conv_rows(A, B, T, Cin, taps=1, stride=1, dil=1, lda=None, a_off=0, a_bstride=None, extra_rows=0):
    """the rows a conv-GEMM reads, gathered from the WHOLE flat array A: element (b, t, tap, k) = A[b a_bstride + a_off + (t stride + tap dil) lda + k]
    -> [B, T, taps, Cin] (extra_rows: that many more rows behind the last tap, as further 'taps' at dilation 1 -- the ConvNeXt prologue's window)"""
    lda = Cin if lda is None else lda
    A = np.asarray(A).reshape(-1)
    b = np.arange(B)[:, None, None, None] * a_bstride
    t = np.arange(T)[None, :, None, None] * stride
    tap = np.concatenate([np.arange(taps) * dil, (taps - 1) * dil + 1 + np.arange(extra_rows)])[None, None, :, None]
    k = np.arange(Cin)[None, None, None, :]
    return A[b + a_off + (t + tap) * lda + k]


def conv_gemm(rows, W, bias=None, act=0, gamma=None, res=None, scale=1.0, c_in=None, a_silu=False, w13=False, rms_w=None, rms_eps=1e-5,
              dw=None, dt=np.float64):
    """rows [B, T, taps, Cin] (conv_rows), W [N, taps Cin] -> [B, T, N] (w13: [B, T, N / 2]):
         v = sum_{tap, k} A'[b, t, tap, k] W[n, tap Cin + k],  A' = silu(A) | A rms_w rsqrt(mean_k A^2 + eps) (taps = 1) |
             LayerNorm(dwconv7(x)) (dw = (wT [7, Cin], b, ln_w, ln_b, eps); rows then holds the 7 window rows of x)
         then + bias, GELU (act 1) or log(max(v, 1e-5)) (act 2), * gamma, + res, * scale, + c_in (accumulate) -- in that order;
         w13: W rows interleave 16 x w1 | 16 x w3, column 16 g + c = silu(v[32 g + c]) v[32 g + 16 + c], no other stage.
    float32: sequential rank-1 updates over k = tap Cin + c ascending, float32 exp / erf, the log as log2(x) * float32(ln 2) (the fast intrinsic)"""
    rows = np.asarray(rows, dt)
    Bn, T, taps, Cin = rows.shape
    if dw is not None:
        wT, db, lw, lb, eps = dw
        assert taps == 7
        x = rows.reshape(Bn * T, 7, Cin)                                  # dwconv7_ln over each row's own window: [rows, 7, C] -> one output row
        a = dwconv7_ln(x, wT, db, lw, lb, eps, dt)[:, 0].reshape(Bn, T, Cin)
    else:
        a = rows
        if a_silu:
            a = silu(a, dt)
        if rms_w is not None:
            assert taps == 1
            a = rms_norm(a[:, :, 0], rms_w, rms_eps, dt)
        a = a.reshape(Bn, T, -1)
    v = _matmul(a, np.asarray(W, dt).T, dt)
    if w13:
        N = v.shape[-1]
        g = v.reshape(Bn, T, N // 32, 2, 16)
        return (silu(g[..., 0, :], dt) * g[..., 1, :]).reshape(Bn, T, N // 2)
    if bias is not None:
        v = v + np.asarray(bias, dt)
    if act == 1:
        v = gelu_erf(v, dt)
    elif act == 2:
        v = np.maximum(v, dt(LOG_CLAMP))
        v = np.log2(v) * dt(np.float32(np.log(2.0))) if dt == np.float32 else np.log(v)
    if gamma is not None:
        v = v * np.asarray(gamma, dt)
    if res is not None:
        v = v + np.asarray(res, dt)
    v = v * dt(np.float32(scale))
    if c_in is not None:
        v = v + np.asarray(c_in, dt)
    return v.astype(dt)


# ---- fp16 planes (csrc/planes_split.h) ---------------------------------------------------------------------------------------------
def h3_split(x):
    """(hi, lo) = (fp16(x), fp16(x - hi)) as float32 values -- csrc/planes_split.h h3_split"""
    x = np.asarray(x, np.float32)
    hi = round_f16(x)
    return hi, round_f16(x - hi)


def weight_planes(W, n_planes):
    """the weights as make_weight_planes holds them: parts of W 2^e, e = 8 - exponent(max |W|) (max |W| 2^e in [2^7, 2^8)), times 2^-e;
    -> (hi, lo) float64 arrays (lo = 0 for one plane)"""
    W = np.asarray(W, np.float32)
    mx = float(np.abs(W).max())
    e = 8 - int(np.frexp(np.float32(mx))[1]) if mx > 0 else 0
    hi, lo = h3_split(W * np.float32(2.0 ** e))
    inv = 2.0 ** -e
    return hi.astype(np.float64) * inv, (lo.astype(np.float64) * inv if n_planes == 2 else np.zeros(W.shape))


def bf16_split3(x):
    """(hi, mid, lo) bf16 parts of float32 x, each rounded to nearest even from the exact residual -- csrc/gemm_split.hip split2"""
    def rne(v):
        u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    x = np.ascontiguousarray(x, np.float32)
    hi = rne(x)
    r1 = (x - hi).astype(np.float32)
    mid = rne(r1)
    r2 = (r1 - mid).astype(np.float32)
    return hi, mid, rne(r2)


def planes_decode(planes, n_planes, rows, K, blocked):
    """planes uint16 [n_planes, rows * K] -> float32 [rows, K] = hi (+ lo).  blocked: element (row, k) at ((k / 32) * rows + row) * 32 + k % 32,
    else row-major"""
    out = np.zeros((rows, K), np.float64)
    for p in range(n_planes):
        f = np.asarray(planes[p], np.uint16).view(np.float16).astype(np.float64)
        out += f.reshape(K // 32, rows, 32).transpose(1, 0, 2).reshape(rows, K) if blocked else f.reshape(rows, K)
    return out


# ---- the tail of the AR decode: sampler, decode GEMV, token and history kernels (csrc/kernels.h, csrc/ar_device.h) ------------------------
def nucleus_token(logits, noise, temperature, top_p):
    """logits_to_probs + multinomial_sample_one_no_sync in float64: softmax; order by descending p, smaller id first; inclusive cumulative sum;
    entries with cum > top_p removed, rank 0 kept; softmax at max(temperature, 1e-5); argmax of p / noise, ties to the smaller id.
    -> (token, decidable, lead).  A row is DECIDABLE when float32 rounding inside a kernel cannot change its winner:
      - the winner is the same with top_p moved by a relative 2e-6 either way (the float32 softmax and its cumulative sum against the threshold),
      - and with the cut moved by one id either way when it falls inside a class of tied probabilities (n p by repeated addition),
      - and the winning ratio leads the runner-up of the kept set by more than 1e-4 relative (lead = best / second; float32 exp and divide)."""
    l, q = np.asarray(logits, np.float64), np.asarray(noise, np.float64)
    V = l.size
    with np.errstate(under="ignore"):
        p = np.exp(l - l.max())
        p = p / p.sum()
        score = np.exp((l - l.max()) / max(float(temperature), 1e-5)) / q          # the temperature softmax up to its (positive) normaliser
    order = np.lexsort((np.arange(V), -p))
    ps = p[order]
    cum = np.cumsum(ps)

    def n_kept(tp):
        return max(int(np.searchsorted(cum, tp, side="right")), 1)              # entries with cum <= tp; rank 0 always

    def winner(n):
        ids = order[:n]
        s = score[ids]
        return int(ids[s == s.max()].min())

    tp = float(np.float32(top_p))                                               # the launchers take a float
    n = n_kept(tp)
    tok = winner(n)
    trials = [n_kept(tp * (1 + 2e-6)), n_kept(tp * (1 - 2e-6))]
    if n < V and ps[n] == ps[n - 1]:
        trials += [n + 1] + ([n - 1] if n >= 2 else [])
    s = np.sort(score[order[:n]])
    lead = float("inf") if n == 1 or s[-2] == 0 else float(s[-1] / s[-2])
    return tok, all(winner(k) == tok for k in trials) and lead > 1 + 1e-4, lead


def swiglu_rows(n_feat):
    """weight rows (w1, w3) of SwiGLU feature f in the 16-row interleave Packer::w13 writes (csrc/packer.hip): group g of 32 rows = w1 rows
    16 g .. 16 g + 15, then w3 rows 16 g .. 16 g + 15"""
    f = np.arange(n_feat)
    r1 = (f >> 4) * 32 + (f & 15)
    return r1, r1 + 16


def pack_w13(w1, w3):
    """[2 I, D] as Packer::w13 interleaves w1 [I, D] and w3 [I, D] (I % 16 == 0)"""
    I, Dm = w1.shape
    return np.stack([np.asarray(w1).reshape(I // 16, 16, Dm), np.asarray(w3).reshape(I // 16, 16, Dm)], 1).reshape(2 * I, Dm)


def gemv_ref(x, W, norm_w=None, eps=1e-5, bias=None, res=None, swiglu=False, half=False, dt=np.float64):
    """the decode GEMV (launch_gemv modes 0 / 1, ardev::gemv): y = (RMSNorm(x) norm_w | x) W^T, then + bias + res, or -- swiglu, W = pack_w13 --
    silu(y[w1 row f]) y[w3 row f] per feature f.  half: the weights as the fp16 fragments hold them."""
    W = round_f16(W) if half else W
    a = rms_norm(x, norm_w, eps, dt) if norm_w is not None else np.asarray(x, dt)
    v = _matmul(a, np.asarray(W, dt).T, dt)
    if swiglu:
        r1, r3 = swiglu_rows(v.shape[-1] // 2)
        return silu(v[..., r1], dt) * v[..., r3]
    if bias is not None:
        v = v + np.asarray(bias, dt)
    if res is not None:
        v = v + np.asarray(res, dt)
    return v


def logit_edits(row, prev, suppress, penalty, W=None, prev_cap=4096):
    """launch_logit_edits on one float32 row, in float32 (one multiply or one divide per listed token, from the ORIGINAL score, each token once):
    prev[: min(W, prev_cap)] with negative and >= V entries skipped: s < 0 ? s * penalty : s / penalty; then suppress ids in [0, V) -> -inf"""
    row = np.array(row, np.float32)
    V = row.size
    prev = np.asarray(prev, np.int64).reshape(-1)
    ids = prev[:max(min(len(prev) if W is None else W, prev_cap), 0)]
    ids = np.unique(ids[(ids >= 0) & (ids < V)])
    sc = row[ids].copy()
    with np.errstate(over="ignore"):
        row[ids] = np.where(sc < 0, sc * np.float32(penalty), sc / np.float32(penalty))
    sup = np.asarray(suppress, np.int64).reshape(-1)
    row[sup[(sup >= 0) & (sup < V)]] = -np.inf
    return row


def audio_embed(table, codes, codebook_size):
    """codes [rows, ncb] -> float32 sum over codebooks of table[code_i + i codebook_size], added in codebook order from 0"""
    acc = np.zeros((codes.shape[0], table.shape[1]), np.float32)
    for i in range(codes.shape[1]):
        acc = acc + np.asarray(table, np.float32)[np.asarray(codes)[:, i] + i * codebook_size]
    return acc


def shift_history(x, H, T):
    """x [..., >= H + T rows, C]: rows [T, T + H) move to [0, H), everything else stays"""
    out = np.array(x)
    out[..., :H, :] = x[..., T:T + H, :]
    return out


def ring_write(ring, chunk, step):
    """chunk [B, n] into ring [B, N] at ((step n) % N + i) % N"""
    out = np.array(ring)
    n, N = chunk.shape[1], ring.shape[1]
    out[:, (step * n + np.arange(n)) % N] = chunk
    return out


# ---- the chunk step's bookkeeping kernels (csrc/engine_kernels.hip): integer and copy models, exact -----------------------------------------
def ring_append(hist, count, new):
    """hist [B, cap] (cap a power of two), count [B], new [B, n]: entry (count[b] + i) mod cap of ring b <- new[b, i] -> (hist, count + n)
    (append_content / put_codes; one codebook row of ar_finish_frame)"""
    hist, count, new = np.array(hist), np.array(count), np.asarray(new)
    cap = hist.shape[-1]
    for b in range(hist.shape[0]):
        for i in range(new.shape[1]):
            hist[b, (int(count[b]) + i) % cap] = new[b, i]
    return hist, count + new.shape[1]


def ring_window(hist_row, end, n):
    """the n entries in front of counter `end` of one ring row, oldest first: what a list that grew to `end` entries holds at [end - n, end)"""
    cap = hist_row.shape[-1]
    return hist_row[..., (end - n + np.arange(n)) % cap]


def finish_frame(tok, last_pos, nframes, pred_hist, step_audio, ci, last_pos_inc):
    """tok [B, ncb] -> pred_hist [B, ncb, cap] at nframes mod cap, step_audio [B, ncb, chunk] column ci; nframes + 1, last_pos + last_pos_inc"""
    pred_hist, step_audio = np.array(pred_hist), np.array(step_audio)
    for q in range(tok.shape[1]):
        pred_hist[:, q], _ = ring_append(pred_hist[:, q], nframes, tok[:, q:q + 1])
    step_audio[:, :, ci] = tok
    return np.asarray(last_pos) + last_pos_inc, np.asarray(nframes) + 1, pred_hist, step_audio


def apply_forced(raw, forced, use_forced, ci, cb, tok):
    """tok [B, ncb]: column cb <- forced[:, cb, ci] when use_forced else raw[:, cb]; the other columns stay"""
    tok = np.array(tok)
    tok[:, cb] = forced[:, cb, ci] if use_forced else raw[:, cb]
    return tok


def prepare_step(cached_audio_emb, content_emb, codes, code_off, last_pos, step_content, ci):
    """decode_one's two tokens per stream: x rows (2 b, 2 b + 1) = (cached_audio_emb[b], content_emb[codes[b, code_off]]) in slot b at
    positions last_pos[b] + 1, + 2 -> (x [2 B, D], slot [2 B], pos [2 B], step_content with column ci = the code)"""
    B = codes.shape[0]
    code = np.asarray(codes)[:, code_off]
    x = np.stack([cached_audio_emb, content_emb[code]], axis=1).reshape(2 * B, -1)
    slot = np.repeat(np.arange(B), 2)
    pos = (np.asarray(last_pos)[:, None] + np.array([1, 2])).reshape(-1)
    step_content = np.array(step_content)
    step_content[:, ci] = code
    return x, slot, pos, step_content


def prompt_rows(content_emb, codebook_emb, wait4start, cc, ac, d, codebook_size):
    """the rows of DualAR.prefill_prompt behind the speaker prefix, R frames: row 2 i = content_emb[cc[i]], row 2 i + 1 = wait4start[i] for i < d,
    else the in-order float32 codebook sum of frame i - d -> (rows [2 R, D], cached_ref_emb [d, D] = the embeddings of the last d frames)"""
    cc, ac = np.asarray(cc), np.asarray(ac)
    R = cc.shape[0]
    emb = audio_embed(codebook_emb, ac[:, :R].T, codebook_size)
    rows = np.empty((2 * R, content_emb.shape[1]), np.float32)
    rows[0::2] = content_emb[cc]
    for i in range(R):
        rows[2 * i + 1] = wait4start[i] if i < d else emb[i - d]
    return rows, emb[R - d:]


def delayfill_rows(content_emb, content_hist, ncontent, cached_ref_emb, last_pos, d, slot_list):
    """prefill_src_condition4delay per listed slot: [c_0, r_0, ..., c_{d-1}] with c = the slot's last d content codes (ring), r = cached_ref_emb
    -> (x [n (2 d - 1), D], slot, pos = last_pos + 1 + r, cached_new_audio_emb per listed slot [n, D] = r_{d-1})"""
    xs, slots, poss, cna = [], [], [], []
    for b in slot_list:
        codes = ring_window(content_hist[b], int(ncontent[b]), d)
        seq = np.stack([content_emb[codes], cached_ref_emb[b, :d]], axis=1).reshape(2 * d, -1)
        cna.append(seq[-1])
        xs.append(seq[:-1])
        slots += [b] * (2 * d - 1)
        poss += [int(last_pos[b]) + 1 + r for r in range(2 * d - 1)]
    return np.concatenate(xs).astype(np.float32), np.array(slots), np.array(poss), np.stack(cna).astype(np.float32)


def _reprefill_audio(pred_hist_b, ref_tail_b, Rt, nf, na):
    """the concatenated audio codes [ref (its last max_delay frames are known), the last na predicted frames] as a dict frame -> codes [ncb]"""
    md = ref_tail_b.shape[1]
    ac = {Rt - md + k: ref_tail_b[:, k] for k in range(md) if Rt - md + k >= 0}        # (the upload leaves the entries in front of frame 0 unset)
    new = ring_window(pred_hist_b, nf, na)
    ac.update({Rt + k: new[:, k] for k in range(na)})
    return ac


def reprefill_rows(content_emb, codebook_emb, wait4start, content_hist, pred_hist, ref_tail, slots, Rt, nf, na, ncon, d, codebook_size, nspk):
    """the re-prefill of StreamSession.process_one_chunk seen from the rings: per due slot the rows of frames Rt .. Rt + na - 1 of
    prefill_prompt([ref, src_content[-na - d:-d]], [ref_audio, pred[-na:]]) (everything in front is the cached prefix) -> (x, slot_out, pos_out)"""
    xs, so, po = [], [], []
    for b, R0, f, a, c in zip(slots, Rt, nf, na, ncon):
        ac = _reprefill_audio(pred_hist[b], ref_tail[b], R0, f, a)
        cont = ring_window(content_hist[b], c - d, a)
        for k in range(a):
            i = R0 + k
            xs.append(content_emb[cont[k]])
            xs.append(wait4start[i] if i < d else audio_embed(codebook_emb, ac[i - d][None], codebook_size)[0])
            so += [b, b]
            po += [nspk + 2 * i, nspk + 2 * i + 1]
    return np.stack(xs).astype(np.float32), np.array(so), np.array(po)


def reprefill_finish(codebook_emb, pred_hist, ref_tail, slots, Rt, nf, na, d, codebook_size, nspk):
    """cached_ref_emb [n, d, D] = the embeddings of the new prompt's last d audio frames, last_pos [n] = its last position"""
    embs, lps = [], []
    for b, R0, f, a in zip(slots, Rt, nf, na):
        ac = _reprefill_audio(pred_hist[b], ref_tail[b], R0, f, a)
        embs.append(audio_embed(codebook_emb, np.stack([ac[R0 + a - d + k] for k in range(d)]), codebook_size))
        lps.append(nspk + 2 * (R0 + a) - 1)
    return np.stack(embs), np.array(lps)


def copy_tokens(tok, d2c, Ht, gap, c):
    """tok [B, >= Ht + gap + c, D]: rows [0, Ht) -> d2c rows [0, Ht), rows [Ht + gap, Ht + gap + c) -> the last c rows of d2c [B, T2, D]"""
    out = np.array(d2c)
    out[:, :Ht] = tok[:, :Ht]
    out[:, out.shape[1] - c:] = tok[:, Ht + gap:Ht + gap + c]
    return out


def mean3(a, b, c):
    """ParallelBlock's mean of the three branches as the kernel evaluates it: ((a + b) + c) / 3 in float32"""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    return ((a + b) + c) / np.float32(3.0)


# ---- fused HiFiGAN level (csrc/voc_fused.hip) ---------------------------------------------------------------------------------------------
VOC_LEVEL_K = (3, 7, 11)


def _causal_conv_rows(x, w, b, k, dil, dt):
    """x [B, N, C] -> bias + sum over taps t of x[r - (k - 1 - t) dil] @ w[:, t C:(t + 1) C].T, rows in front of the array read as zero"""
    B, N, C = x.shape
    xp = np.concatenate([np.zeros((B, (k - 1) * dil, C), dt), x], axis=1)
    acc = np.broadcast_to(np.asarray(b, dt), (B, N, w.shape[0])).copy()
    for t in range(k):
        acc = acc + _matmul(xp[:, t * dil:t * dil + N], np.asarray(w[:, t * C:(t + 1) * C], dt).T, dt)
    return acc


def voc_level(x_hist_and_new, W, bias, dil, frames_before, dt=np.float64, hist=None):
    """The three ResBlock1 branches y += c2(silu(c1(silu(y)))) for the three dilations, kernel sizes 3 / 7 / 11, over x_hist_and_new [B, hist + T, C]
    (`hist` history rows -- default: the chain's receptive field 20 sum(dil), what the kernel asks for -- then T new rows; channel-last).
    W[br][q] [C, k C] with column t C + c = tap t, input channel c (q = 2 j: conv 1 of dilation j, 2 j + 1: conv 2), bias[br][q] [C].
    `frames_before` = stream rows in front of the first new row: every conv's input is zero on the left of the stream start, so history rows in
    front of it are never read (they may hold anything) and every intermediate is zero there; history rows inside the stream are used -> [3, B, T, C]"""
    hist = 20 * sum(dil) if hist is None else hist
    x = np.array(x_hist_and_new, dtype=dt)
    outside = np.arange(x.shape[1]) < hist - frames_before          # rows in front of the stream start
    x[:, outside] = 0
    out = []
    for br, k in enumerate(VOC_LEVEL_K):
        assert hist >= (k - 1) * 2 * sum(dil)
        y = x.copy()
        for j, dl in enumerate(dil):
            t = _causal_conv_rows(silu(y, dt), W[br][2 * j], bias[br][2 * j], k, dl, dt)
            t[:, outside] = 0
            t = _causal_conv_rows(silu(t, dt), W[br][2 * j + 1], bias[br][2 * j + 1], k, dl, dt)
            t[:, outside] = 0
            y = (t + y).astype(dt)
        out.append(y[:, hist:])
    return np.stack(out)


# ---- one conv stage of a narrow HiFiGAN level over dense rows (csrc/gemm_planes.hip: voc_conv_kernel; csrc/sva_common.h: VocConv) -----------
def voc_conv_ref(rows, W, bias, res, taps, dil, a_row0=0, T=None, dt=np.float64):
    """rows [B, a_rows, C]: the dense input rows of every stream AS THE CONV READS THEM (SiLU is the producer's: the planes hold silu(.)), history in
    front; W [N, taps C] with column j C + c = tap j, input channel c; bias [N] or None; res [B, T, N] or None.  The causal dilated conv
        v[b, t] = sum_j rows[b, a_row0 + t + j dil] @ W[:, j C:(j + 1) C].T + bias (+ res[b, t]),  t = 0 .. T - 1
    (output row t sits at input row a_row0 + t + (taps - 1) dil: the last tap reads the row itself, the first one (taps - 1) dil rows back)
    -> (v, silu(v)), both [B, T, N]: the fp32 output and what the kernel's output planes hold.
    float32: one rank-1 update per k = j C + c in ascending order, then the bias, then the residual"""
    rows = np.asarray(rows, dt)
    B, n_rows, C = rows.shape
    T = n_rows - a_row0 - (taps - 1) * dil if T is None else T
    assert a_row0 >= 0 and T >= 1 and a_row0 + T + (taps - 1) * dil <= n_rows and np.shape(W) == (np.shape(W)[0], taps * C)
    a = np.concatenate([rows[:, a_row0 + j * dil:a_row0 + j * dil + T] for j in range(taps)], axis=-1)          # [B, T, taps C]
    v = _matmul(a, np.asarray(W, dt).T, dt)
    if bias is not None:
        v = v + np.asarray(bias, dt)
    if res is not None:
        v = v + np.asarray(res, dt)
    v = v.astype(dt)
    return v, silu(v, dt)
