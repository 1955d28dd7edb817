"""NumPy restatements of the non-GEMM operations, written from their definitions (csrc/kernels.h, oracle/sva_oracle.py), for the
per-kernel GPU tests (test_gpu_kernels.py).  tests/test_kernel_refs.py pins each of them to the oracle's own function on the CPU.

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


# ---- fp16 planes (csrc/planes_split.h) ---------------------------------------------------------------------------------------------
def planes_decode(planes, n_planes, rows, K, blocked):
    """planes uint16 [n_planes, rows * K] -> float32 [rows, K] = hi (+ lo).  blocked: element (row, k) at ((k / 32) * rows + row) * 32 + k % 32,
    else row-major"""
    out = np.zeros((rows, K), np.float64)
    for p in range(n_planes):
        f = np.asarray(planes[p], np.uint16).view(np.float16).astype(np.float64)
        out += f.reshape(K // 32, rows, 32).transpose(1, 0, 2).reshape(rows, K) if blocked else f.reshape(rows, K)
    return out
