"""Every non-GEMM HIP kernel, alone, through its production launcher (the sva_test_* hooks of csrc/testhooks.hip), against the float64
references of tests/kernel_refs.py at the shapes, strides and positions where its dispatch changes.

Bounds are derived on the CPU, never fitted to the kernel: e32 = max |f32ref - f64ref| with f32ref the same formula evaluated naively in
NumPy float32 (sequential sums), and max |kernel - f64ref| <= 4 e32 + 4 ulp32(max |f64ref|) -- the factor 4 the GEMM tests use for "fp32,
another summation order".  Where the float32 restatement of a large case is taken on a sub-tensor (first batch item / first head) e32 can
only be smaller, the bound only tighter.  Wider terms are derived from a named cause next to the case (fp16 planes, fp16 cache rounding).
Exact where the operation is exact: indices, untouched rows / cache entries (a sentinel), zeroed pads, RoPE at position 0, copied V rows.
No attention output may exceed the 2e-5 of test_prefill_attention_mfma_vs_fp64 (same input scale); no BSQ u the 2e-5 of the module docstring.

With SVA_KERNEL_PARITY_TABLE=<path> the run writes its table (kernel, shape, error, bound, ratio) there (profiles/kernel_parity.txt)."""
import hashlib
import os
import time

import numpy as np
import pytest

import kernel_refs as R

pytestmark = pytest.mark.gpu

SENT = 777.0
_TABLE = []
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    t0 = time.time()
    yield
    path = os.environ.get("SVA_KERNEL_PARITY_TABLE")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("# %d cases, worst err / bound = %.3f, wall %.1f s\n" % (len(_TABLE), max(r[4] for r in _TABLE), time.time() - t0))
            f.write("%-34s %-58s %12s %12s %8s\n" % ("kernel", "shape", "max_err", "bound", "ratio"))
            for k, s, e, b, r in _TABLE:
                f.write("%-34s %-58s %12.4e %12.4e %8.3f\n" % (k, s, e, b, r))


def _E():
    from streamvoiceanon_amd import engine as E
    return E


def digest(kernel, tag, got):
    """bit identity between two builds of the library: with SVA_KERNEL_DIGESTS=PATH every compared output appends
    `kernel, tag, sha1(its bytes)` to that file; run the same tests under both builds (SVA_LIB_PATH) and compare the sorted files"""
    path = os.environ.get("SVA_KERNEL_DIGESTS")
    if path:
        with open(path, "a") as f:
            f.write("%s, %s, %s\n" % (kernel, tag, hashlib.sha1(np.ascontiguousarray(got).tobytes()).hexdigest()))


def _check(record_property, kernel, shape, got, f64, f32=None, extra=0.0, ceiling=None, e32=None):
    """the one floating comparison of this file: err <= min(4 e32 + 4 ulp32(max |ref|) + extra, ceiling); e32 from the float32 restatement
    `f32` of the same elements, or handed in when it was taken on a sub-tensor"""
    digest(kernel, shape, got)
    got, f64 = np.asarray(got, F64), np.asarray(f64, F64)
    assert got.shape == f64.shape, (kernel, shape, got.shape, f64.shape)
    e32 = R.e32_of(f32, f64) if e32 is None else e32
    bnd = R.bound(e32, f64, extra)
    if ceiling is not None:
        bnd = min(bnd, ceiling)
    assert np.isfinite(got).all(), (kernel, shape, "non-finite output")
    err = float(np.abs(got - f64).max())
    ratio = err / bnd
    _TABLE.append((kernel, str(shape), err, bnd, ratio))
    record_property("err_over_bound", dict(kernel=kernel, shape=str(shape), err=err, bound=bnd, e32=e32, ratio=ratio))
    print("%s %s err %.3e bound %.3e (e32 %.3e) ratio %.3f" % (kernel, shape, err, bnd, e32, ratio))
    assert err <= bnd, (kernel, shape, err, bnd)


def _exact(kernel, shape, ok, what):
    _TABLE.append((kernel, str(shape) + " " + what, 0.0 if ok else 1.0, 0.0, 0.0 if ok else float("inf")))
    assert ok, (kernel, shape, what)


def _last_error():
    return _E().load_library().sva_last_error().decode("utf-8", "replace")


# =====================================================================================================================================
# decode attention family
# =====================================================================================================================================
EDGE_POS = lambda S: [0, 1, 7, 8, 63, 64, 65, 255, 256, 1023, S - 2, S - 1]      # block / wave boundaries of the key loops


def _filled_cache(n_slots, H, S):
    """every entry +-1e4 (finite in fp16 too): a kernel that reads one key too many lets it dominate the softmax"""
    c = np.empty((n_slots, 2, H, S, 64), F32)
    c[..., 0::2] = 1e4
    c[..., 1::2] = -1e4
    return c


def _valid_rows(rng, cache, slot, upto, half):
    """asymmetric K / V (per-head offsets, V shifted) in keys 0 .. upto of `slot`"""
    H = cache.shape[2]
    k = rng.standard_normal((H, upto + 1, 64)) + 0.05 * np.arange(H)[:, None, None]
    v = rng.standard_normal((H, upto + 1, 64)) + 0.25 + 0.1 * np.arange(64)[None, None, :] / 64
    cache[slot, 0, :, :upto + 1] = R.round_f16(k) if half else k
    cache[slot, 1, :, :upto + 1] = R.round_f16(v) if half else v


def _q_rows(rng, M, H):
    qkv = np.zeros((M, 3 * H * 64), F32)
    qkv[:, :H * 64] = rng.standard_normal((M, H * 64)) * 1.5 + 0.02 * np.arange(H * 64) / (H * 64)
    return qkv


def _run_attention_case(record_property, variant, half, H, S, slots_pos, n_slots, seed, tag):
    """slots_pos: [(slot, pos)] one per row (variant 0) or per PAIR (variant 2: rows at pos, pos + 1)"""
    E = _E()
    rng = np.random.default_rng(seed)
    cache = _filled_cache(n_slots, H, S)
    slot, pos = [], []
    for s, p in slots_pos:
        _valid_rows(rng, cache, s, p + (1 if variant == 2 else 0), half)
        slot += [s, s] if variant == 2 else [s]
        pos += [p, p + 1] if variant == 2 else [p]
    M = len(slot)
    qkv = _q_rows(rng, M, H)
    before = cache.copy()
    out, qkv2, cache2 = E.test_decode_attention(variant, qkv, cache, slot, pos, half_kv=half, out_fill=SENT)
    name = ("ar_attention_pair" if variant == 2 else "ar_attention") + ("<half>" if half else "<float>")
    shape = "%s M=%d H=%d S=%d slots=%d" % (tag, M, H, S, n_slots)
    _exact(name, shape, np.array_equal(cache2, before) and np.array_equal(qkv2, qkv), "inputs untouched")
    want = R.decode_attention(qkv[:, :H * 64], cache, slot, pos, H)
    want32 = R.decode_attention(qkv[:, :H * 64], cache, slot, pos, H, F32)
    _check(record_property, name, shape, out, want, want32, ceiling=2e-5)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("variant", [0, 2])
def test_decode_attention_edge_positions_product_shape(variant, half, record_property):
    """H = 12, S = 2048 (the engine's slow cache): one row (pair) per slot, slots shuffled, every edge position of the key loop; for pairs
    (p, p + 1) straddles each edge from both sides"""
    H, S = 12, 2048
    if variant == 2:
        starts = sorted({min(max(p + d, 0), S - 2) for p in EDGE_POS(S) for d in (-1, 0)})
    else:
        starts = EDGE_POS(S)
    rng = np.random.default_rng(11 + variant)
    slots = rng.permutation(len(starts))
    _run_attention_case(record_property, variant, half, H, S, list(zip(slots.tolist(), starts)), len(starts), 100 + variant + 2 * half, "edges")


@pytest.mark.parametrize("n_slots,half", [(1, False), (1, True), (3, False), (3, True), (64, True), (128, False)])
@pytest.mark.parametrize("variant", [0, 2])
def test_decode_attention_shuffled_slots_ragged_positions(variant, n_slots, half, record_property):
    """a running batch: one row (pair) per slot in a shuffled slot order, ragged positions drawn from the edge list; H = 12 for 1 and 3 slots,
    H = 2 for 64 and 128 (the cache of 128 x 12 heads x 2048 keys would be 1.6 GB of test data).  Thinned for run time: 64 slots with the fp16
    cache, 128 with the fp32 one; every edge position stays"""
    H, S = (12, 2048) if n_slots <= 3 else (2, 2048)
    rng = np.random.default_rng(1000 + n_slots + variant)
    edges = [min(p, S - 2) for p in EDGE_POS(S)] if variant == 2 else EDGE_POS(S)
    poss = [edges[i] for i in rng.permutation(n_slots) % len(edges)]
    if n_slots == 1:
        poss = [S - 2 if variant == 2 else S - 1]
    slots = rng.permutation(n_slots).tolist()
    _run_attention_case(record_property, variant, half, H, S, list(zip(slots, poss)), n_slots, 2000 + n_slots + variant + 7 * half, "ragged")


def test_decode_attention_hook_refuses_rows_outside_the_cache():
    E = _E()
    cache = np.zeros((2, 2, 1, 16, 64), F32)
    qkv = np.zeros((2, 192), F32)
    for slot, pos in (([0, 2], [1, 1]), ([0, 1], [1, 16]), ([0, -1], [0, 0])):
        with pytest.raises(RuntimeError, match="outside the cache"):
            E.test_decode_attention(0, qkv, cache, slot, pos)
    with pytest.raises(RuntimeError, match="pair rows"):
        E.test_decode_attention(2, qkv, cache, [0, 0], [3, 5])


def _wo(rng, D, rows=None):
    """asymmetric projection: a transposed or head-swapped product cannot match"""
    rows = D if rows is None else rows
    return (rng.standard_normal((rows, D)) / np.sqrt(D) + 0.01 * np.arange(rows)[:, None] / rows).astype(F32)


@pytest.mark.parametrize("M", [1, 2])
def test_split_key_attention_merged_by_gemv_mode4(M, record_property):
    """the B <= 2 slow layer: ar_attention_kernel with 8 key splits + gemv_kernel mode 4 (merge, wo, residual) against fp64
    x + W attention; positions below the split count (empty splits), just above it, and at the 16-key rounding of the split length"""
    E = _E()
    H, S, D = 12, 2048, 768
    for i, p0 in enumerate([0, 1, 5, 7, 8, 9, 15, 16, 17, 127, 128, 129, 1023, S - 1]):
        rng = np.random.default_rng(300 + i)
        poss = [p0, [S - 1, 6, 130, 3][i % 4]][:M]
        slot = [1, 0][:M]
        cache = _filled_cache(2, H, S)
        for s, p in zip(slot, poss):
            _valid_rows(rng, cache, s, p, False)
        qkv = _q_rows(rng, M, H)
        x = (rng.standard_normal((M, D)) + 0.5).astype(F32)
        W = _wo(rng, D)
        out, _, cache2 = E.test_decode_attention(1, qkv, cache, slot, poss, x=x, W=W, out_fill=SENT)
        shape = "M=%d pos=%s" % (M, poss)
        _exact("ar_attention split + gemv mode 4", shape, np.array_equal(cache2, cache), "cache untouched")
        att, att32 = R.decode_attention(qkv[:, :D], cache, slot, poss, H), R.decode_attention(qkv[:, :D], cache, slot, poss, H, F32)
        want = x.astype(F64) + att @ W.astype(F64).T
        want32 = x + R._matmul(att32, W.T, F32)
        _check(record_property, "ar_attention split + gemv mode 4", shape, out, want, want32)


@pytest.mark.parametrize("M", [1, 2, 3, 64, 128])
def test_fast_attention_every_codebook_position(M, record_property):
    """ar_fast_attention_kernel: RoPE + cache write + attention over <= 8 keys; every position 0 .. 7 (M < 8: over several seeds)"""
    E = _E()
    H = 12
    tab = R.rope_table(8)
    for rep in range(1 if M >= 8 else 8):
        rng = np.random.default_rng(400 + M + 10 * rep)
        n_slots = max(M, 2)
        # row m sits at one codebook position of its own slot: the keys below it are valid, the rest of the 8-entry cache is +-1e4
        cache = _filled_cache(n_slots, H, 8)
        slot = rng.permutation(n_slots)[:M].tolist()
        pos = [(rep + 3 * m) % 8 for m in range(M)]
        for s, p in zip(slot, pos):
            if p > 0:
                _valid_rows(rng, cache, s, p - 1, False)
        qkv = (rng.standard_normal((M, 3 * H * 64)) * 1.2 + 0.02 * np.arange(3 * H * 64) / (H * 64)).astype(F32)
        out, qkv2, cache2 = E.test_decode_attention(3, qkv, cache, slot, pos, rope=tab, out_fill=SENT)
        shape = "M=%d pos=%s" % (M, pos if M < 8 else "3m mod 8")
        q64, c64 = R.rope_kvwrite(qkv, cache, slot, pos, tab, H)
        q32, c32 = R.rope_kvwrite(qkv, cache, slot, pos, tab, H, dt=F32)
        _exact("ar_fast_attention", shape, np.array_equal(qkv2, qkv), "qkv rows untouched")
        written = np.zeros(cache.shape, bool)
        for s, p in zip(slot, pos):
            written[s, :, :, p] = True
        _exact("ar_fast_attention", shape, np.array_equal(cache2[~written], cache[~written]), "cache outside (slot, pos) untouched")
        _exact("ar_fast_attention", shape, np.array_equal(cache2[:, 1][written[:, 1]], c64[:, 1][written[:, 1]].astype(F32)), "V rows copied exactly")
        _check(record_property, "ar_fast_attention K write", shape, cache2[:, 0][written[:, 0]], c64[:, 0][written[:, 0]], c32[:, 0][written[:, 0]])
        want = R.decode_attention(q64[:, :H * 64], c64, slot, pos, H)
        want32 = R.decode_attention(q32[:, :H * 64], c32, slot, pos, H, F32)
        _check(record_property, "ar_fast_attention", shape, out, want, want32, ceiling=2e-5)


@pytest.mark.parametrize("M", [1, 2])
def test_gemv_mode3_attention_inside_wo(M, record_property):
    """gemv_kernel mode 3 (fast AR at B <= 2): attention of the already rotated q over keys 0 .. pos inside the wo GEMV + residual"""
    E = _E()
    H, D = 12, 768
    for p0 in range(8):
        rng = np.random.default_rng(500 + p0 + 10 * M)
        poss = [p0, (p0 + 5) % 8][:M]
        slot = [2, 0][:M]
        cache = _filled_cache(3, H, 8)
        for s, p in zip(slot, poss):
            _valid_rows(rng, cache, s, p, False)
        qkv = _q_rows(rng, M, H)
        qkv[:, D:] = SENT                       # the k / v columns of the rows are not this kernel's to read
        x = (rng.standard_normal((M, D)) + 0.5).astype(F32)
        W = _wo(rng, D)
        out, _, cache2 = E.test_decode_attention(4, qkv, cache, slot, poss, x=x, W=W, out_fill=SENT)
        shape = "M=%d pos=%s" % (M, poss)
        _exact("gemv mode 3", shape, np.array_equal(cache2, cache), "cache untouched")
        att, att32 = R.decode_attention(qkv[:, :D], cache, slot, poss, H), R.decode_attention(qkv[:, :D], cache, slot, poss, H, F32)
        _check(record_property, "gemv mode 3", shape, out, x.astype(F64) + att @ W.astype(F64).T, x + R._matmul(att32, W.T, F32))


def _check_kv_write(record_property, name, shape, qkv, qkv2, cache, cache2, slot, pos, tab, H, half, q64, q32, c64, c32):
    D = H * 64
    written = np.zeros(cache.shape, bool)
    for s, p in zip(slot, pos):
        written[s, :, :, p] = True
    _exact(name, shape, np.array_equal(cache2[~written], cache[~written]), "whole cache outside (slot, pos) untouched")
    # fp16 cache: the kernel rounds ITS fp32 value, which may sit on the other side of an fp16 rounding boundary than the fp64 one:
    # at most one fp16 ulp of the largest written value
    extra = float(np.spacing(np.float16(np.abs(c64[:, 0][written[:, 0]]).max()))) if half else 0.0
    _check(record_property, name + " K", shape, cache2[:, 0][written[:, 0]], c64[:, 0][written[:, 0]], c32[:, 0][written[:, 0]], extra=extra)
    return written


@pytest.mark.parametrize("half", [False, True])
def test_rope_kvwrite_positions_and_whole_cache(half, record_property):
    """rope_kvwrite_kernel<float | __half>: position 0 is the identity (exact), the last table row, two rows sharing a slot; K / V land at
    exactly (slot, pos): the WHOLE cache is compared"""
    E = _E()
    H, S, D = 12, 2048, 768
    rng = np.random.default_rng(600 + half)
    tab = R.rope_table(S)
    slot, pos = [3, 0, 4, 0, 2, 1], [0, S - 1, 1023, 64, 65, 0]
    cache = R.round_f16(_filled_cache(5, H, S))
    qkv = (rng.standard_normal((len(slot), 3 * D)) + 0.02 * np.arange(3 * D) / D).astype(F32)
    out, qkv2, cache2 = E.test_decode_attention(5, qkv, cache, slot, pos, rope=tab, half_kv=half)
    name, shape = "rope_kvwrite" + ("<half>" if half else "<float>"), "M=6 pos=%s" % pos
    q64, c64 = R.rope_kvwrite(qkv, cache, slot, pos, tab, H, half_kv=half)
    q32, c32 = R.rope_kvwrite(qkv, cache, slot, pos, tab, H, half_kv=half, dt=F32)
    written = _check_kv_write(record_property, name, shape, qkv, qkv2, cache, cache2, slot, pos, tab, H, half, q64, q32, c64, c32)
    _exact(name, shape, np.array_equal(cache2[:, 1][written[:, 1]], c64[:, 1][written[:, 1]].astype(F32)), "V rows exact")
    _exact(name, shape, np.array_equal(qkv2[:, D:], qkv[:, D:]), "k / v columns of the rows untouched")
    for m in (0, 5):       # position 0: cos = 1, sin = 0 exactly
        _exact(name, shape, np.array_equal(qkv2[m, :D], qkv[m, :D]), "q at position 0 unchanged")
        kw = cache2[slot[m], 0, :, 0].reshape(D)
        _exact(name, shape, np.array_equal(kw, R.round_f16(qkv[m, D:2 * D]) if half else qkv[m, D:2 * D]), "k at position 0 unchanged")
    _check(record_property, name + " q", shape, qkv2[:, :D], q64[:, :D], q32[:, :D])


@pytest.mark.parametrize("M", [1, 2])
def test_gemv_mode2_qkv_rope_kvwrite(M, record_property):
    """gemv_kernel mode 2 (B <= 2 decode): RMSNorm prologue, QKV projection, RoPE on q / k, K / V written to (slot, pos)"""
    E = _E()
    H, D = 12, 768
    for S, poss in ((2048, [0, 2047]), (2048, [1023, 64]), (8, [7, 0]), (8, [3, 4])):
        rng = np.random.default_rng(700 + S + poss[0])
        poss, slot = poss[:M], [1, 0][:M]
        tab = R.rope_table(S)
        cache = _filled_cache(2, H, S)
        x = (rng.standard_normal((M, D)) * 2 + 0.3).astype(F32)
        nw = rng.uniform(0.5, 1.5, D).astype(F32)
        W = _wo(rng, D, 3 * D)
        qkv = np.full((M, 3 * D), SENT, F32)
        _, qkv2, cache2 = E.test_decode_attention(6, qkv, cache, slot, poss, rope=tab, x=x, W=W, norm_w=nw)
        shape = "M=%d S=%d pos=%s" % (M, S, poss)
        pre64 = R.rms_norm(x, nw, 1e-5) @ W.astype(F64).T
        pre32 = R._matmul(R.rms_norm(x, nw, 1e-5, F32), W.T, F32)
        q64, c64 = R.rope_kvwrite(pre64, cache, slot, poss, tab, H)
        q32, c32 = R.rope_kvwrite(pre32, cache, slot, poss, tab, H, dt=F32)
        written = _check_kv_write(record_property, "gemv mode 2", shape, qkv, qkv2, cache, cache2, slot, poss, tab, H, False, q64, q32, c64, c32)
        _check(record_property, "gemv mode 2 V", shape, cache2[:, 1][written[:, 1]], c64[:, 1][written[:, 1]], c32[:, 1][written[:, 1]])
        _check(record_property, "gemv mode 2 q", shape, qkv2[:, :D], q64[:, :D], q32[:, :D])
        _exact("gemv mode 2", shape, bool((qkv2[:, D:] == SENT).all()), "k / v columns of Y untouched")


# =====================================================================================================================================
# encoder attention: three kernels, several launch shapes
# =====================================================================================================================================
def _enc_cases():
    cases = []
    for T in (4, 16, 48, 64, 80, 128, 132, 256, 260, 512, 516, 560, 1028):
        for B in (1, 3, 64):
            if B == 64 and T > 128:          # thinned: the large-batch crossings of the long windows (the edges stay)
                continue
            cases.append((T, B, 2 if (T == 1028 and B == 3) else 8, 0))
        rows = {T - 4, T - 16, (T // 32) * 16}
        for row0 in sorted(r for r in rows if 0 < r < T):
            cases.append((T, 3 if T <= 560 else 1, 8, row0))
    cases += [(48, 1, 3, 0), (132, 3, 3, 0), (516, 1, 3, 500), (128, 64, 8, 64), (64, 3, 8, 33), (128, 1, 8, 1)]
    return cases


def _enc_inputs(T, B, H, seed):
    rng = np.random.default_rng(seed)
    D = H * 64
    qkv = rng.standard_normal((B, T, 3 * D)).astype(F32)
    qkv[..., :D] *= 1.5
    qkv[..., 2 * D:] += 0.25 + 0.1 * np.arange(D) / D          # asymmetric V: a head-swapped or transposed write cannot match
    qkv += 0.02 * np.arange(T)[None, :, None] / T
    return qkv


def _enc_refs(qkv, tab, H, T):
    """(fp64 reference, e32 of the float32 restatement on a sub-tensor: the first item; beyond 256 tokens its first head only)"""
    D = H * 64
    want = R.enc_attention(qkv, tab, H)
    if T <= 256:
        return want, R.e32_of(R.enc_attention(qkv[:1], tab, H, dt=F32), want[:1])
    sub = np.concatenate([qkv[:1, :, 0:64], qkv[:1, :, D:D + 64], qkv[:1, :, 2 * D:2 * D + 64]], -1)
    return want, R.e32_of(R.enc_attention(sub, tab, 1, dt=F32), want[:1, :, :64])


@pytest.mark.parametrize("T,B,H,row0", _enc_cases())
def test_enc_attention_vs_fp64(T, B, H, row0, record_property):
    """launch_enc_attention over its whole dispatch: enc_attention_mfma_kernel<4|8> (T % 16 == 0, T <= 128; query splits 1 / 2 / 4),
    enc_attention_kernel (T <= 512; qs 1 .. 8; the row0 > 0 form), enc_attention_flash_kernel (T > 512; with and without a full 512-key
    window).  Causal softmax(q k^T / 8) v, RoPE on q and k, keys max(0, r - 511) .. r; rows below row0 keep the sentinel."""
    E = _E()
    qkv = _enc_inputs(T, B, H, 31 * T + B + H + row0)
    tab = R.rope_table(T)
    out, _ = E.test_enc_attention(qkv, tab, H, row0=row0, fill=SENT)
    shape = "T=%d B=%d H=%d row0=%d" % (T, B, H, row0)
    _exact("enc_attention", shape, bool((out[:, :row0] == SENT).all()), "rows below row0 untouched")
    want, e32 = _enc_refs(qkv, tab, H, T)
    _check(record_property, "enc_attention", shape, out[:, row0:], want[:, row0:], e32=e32, ceiling=2e-5)


@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("T,B,row0", [(16, 1, 0), (48, 3, 0), (64, 64, 0), (80, 3, 0), (128, 1, 0), (128, 3, 112), (128, 3, 124), (96, 64, 64)])
def test_enc_attention_planes_output(T, B, row0, n_planes, record_property):
    """the planes-writing output of the MFMA kernel (K-blocked fp16 hi (+ lo), csrc/planes_split.h) decoded back to fp32.
    Derived widening: hi = fp16(x) is off by at most 2^-11 |x| (+ 2^-25 in the subnormal range); with lo = fp16(x - hi) the sum is off by
    at most 2^-11 |x - hi| <= 2^-22 |x| (+ 2^-25)."""
    E = _E()
    H = 8
    qkv = _enc_inputs(T, B, H, 77 * T + B + row0)
    tab = R.rope_table(T)
    out, planes = E.test_enc_attention(qkv, tab, H, row0=row0, n_planes=n_planes, blocked=True, fill=SENT)
    shape = "T=%d B=%d row0=%d planes=%d" % (T, B, row0, n_planes)
    _exact("enc_attention planes", shape, bool((out == SENT).all()), "fp32 rows untouched when planes are written")
    raw = np.stack([R.planes_decode(planes[p:p + 1], 1, B * T, H * 64, True) for p in range(2)]).reshape(2, B, T, H * 64)
    keep = np.asarray(planes, np.uint16).reshape(2, (H * 64) // 32, B * T, 32).transpose(0, 2, 1, 3).reshape(2, B, T, H * 64)
    _exact("enc_attention planes", shape, bool((keep[:, :, :row0] == 0xFFFF).all()), "plane rows below row0 untouched")
    if n_planes == 1:
        _exact("enc_attention planes", shape, bool((keep[1] == 0xFFFF).all()), "lo plane untouched with one plane")
    got = raw[0] + (raw[1] if n_planes == 2 else 0.0)
    want, e32 = _enc_refs(qkv, tab, H, T)
    amax = float(np.abs(want[:, row0:]).max())
    extra = (2.0 ** -22 if n_planes == 2 else 2.0 ** -11) * amax + 2.0 ** -25
    _check(record_property, "enc_attention planes", shape, got[:, row0:], want[:, row0:], e32=e32, extra=extra, ceiling=(2e-5 if n_planes == 2 else None))


def test_enc_attention_refusals():
    """arguments the launcher cannot serve are refused, not silently mis-served"""
    E = _E()
    tab = R.rope_table(132)
    for T, row0, planes, blocked, msg in ((6, 0, 0, False, "multiple of 4"), (132, 0, 1, True, "planes output only"), (64, 0, 2, False, "K-blocked only"),
                                         (132, 121, 0, False, "partial row range")):
        with pytest.raises(RuntimeError, match=msg):
            E.test_enc_attention(np.zeros((1, T, 192), F32), tab[:T], 1, row0=row0, n_planes=planes, blocked=blocked)
        assert msg in _last_error()


# =====================================================================================================================================
# row operations
# =====================================================================================================================================
ROW_TB = [(1, 1), (3, 2), (4, 64), (10, 2), (170, 1), (171, 2), (10, 64)]


def _rows_index(B, T, C, bstride, off, ld):
    return (np.arange(B)[:, None, None] * bstride + off + np.arange(T)[None, :, None] * ld + np.arange(C)[None, None, :]).astype(np.int64)


def _row_inputs(rng, B, T, C):
    """rows with an offset and a per-channel tilt; row 0 constant (variance 0: eps decides; 0.5 sums exactly in fp32), row 1 scaled by 1e4,
    row 2 by 1e-4 (the mean of squares must neither overflow nor flush)"""
    x = (rng.standard_normal((B * T, C)) * 1.5 + 0.3 + 0.2 * np.arange(C) / C).astype(F32)
    x[0] = 0.5
    if B * T > 1:
        x[1] *= 1e4
    if B * T > 2:
        x[2] *= 1e-4
    return x.reshape(B, T, C)


def _scatter(vals, idx, n, fill=0.0):
    flat = np.full(n, fill, F32)
    flat[idx] = vals
    return flat


@pytest.mark.parametrize("T,B", ROW_TB)
@pytest.mark.parametrize("C", [128, 256, 384, 512, 768])
@pytest.mark.parametrize("kind", [1, 2])
def test_norm_rows_strided(kind, C, T, B, record_property):
    """norm_rows_kernel through launch_layernorm_rows (kind 1, with skip ranges) and launch_rmsnorm_rows (kind 2): ldx != C, non-zero offsets,
    batch strides larger than the tensor; everything outside the written rows keeps the sentinel"""
    E = _E()
    rng = np.random.default_rng(kind * 100000 + C * 100 + T + B)
    ldx, ldo, x_off, o_off = C + 8, C + 24, 40, 16
    xb, ob = T * ldx + 72, T * ldo + 56
    xi, oi = _rows_index(B, T, C, xb, x_off, ldx), _rows_index(B, T, C, ob, o_off, ldo)
    x = _row_inputs(rng, B, T, C)
    w = rng.uniform(0.5, 1.5, C).astype(F32)
    b = rng.standard_normal(C).astype(F32)
    xflat = _scatter(x, xi, (B - 1) * xb + x_off + T * ldx, fill=1e30)         # gaps hold a value that would wreck any row that read them
    skips = [(0, 0)] if kind == 2 else [(0, 0), (1, min(3, T)), (0, T), (T // 2, T // 2)]
    for skip in skips:
        out = np.full((B - 1) * ob + o_off + T * ldo + 5, SENT, F32)
        eps = 1e-5 if kind == 2 else 1e-6
        E.test_rowop(kind, xflat, B, T, C, [w, b] if kind == 1 else [w], eps, out, xb, x_off, ldx, ob, o_off, ldo, skip=skip)
        name = "layernorm_rows" if kind == 1 else "rmsnorm_rows"
        shape = "C=%d T=%d B=%d skip=%s" % (C, T, B, skip)
        live = np.ones(T, bool)
        live[skip[0]:skip[1]] = False
        written = np.zeros(out.size, bool)
        written[oi[:, live].reshape(-1)] = True
        _exact(name, shape, bool((out[~written] == SENT).all()), "outside the written rows untouched")
        if not live.any():
            continue
        ref = (lambda dt: R.layer_norm(x, w, b, eps, dt)) if kind == 1 else (lambda dt: R.rms_norm(x, w, eps, dt))
        _check(record_property, name, shape, out[oi][:, live], ref(F64)[:, live], ref(F32)[:, live])


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("C,T,B", [(512, 10, 2), (512, 171, 2), (768, 4, 64), (128, 3, 1)])
def test_rmsnorm_rows_planes_output(C, T, B, n_planes, blocked, record_property):
    """planes output of launch_rmsnorm_rows vs hi + lo (widening derived as in test_enc_attention_planes_output)"""
    E = _E()
    rng = np.random.default_rng(C + T + B)
    x = _row_inputs(rng, B, T, C)
    w = rng.uniform(0.5, 1.5, C).astype(F32)
    out = np.full(B * T * C, SENT, F32)
    _, planes = E.test_rowop(2, x, B, T, C, [w], 1e-5, out, T * C, n_planes=n_planes, blocked=blocked)
    shape = "C=%d T=%d B=%d planes=%d blocked=%d" % (C, T, B, n_planes, blocked)
    _exact("rmsnorm_rows planes", shape, bool((out == SENT).all()), "fp32 rows untouched when planes are written")
    if n_planes == 1:
        _exact("rmsnorm_rows planes", shape, bool((planes[1] == 0xFFFF).all()), "lo plane untouched with one plane")
    got = R.planes_decode(planes, n_planes, B * T, C, blocked).reshape(B, T, C)
    want = R.rms_norm(x, w, 1e-5)
    extra = (2.0 ** -22 if n_planes == 2 else 2.0 ** -11) * float(np.abs(want).max()) + 2.0 ** -25
    _check(record_property, "rmsnorm_rows planes", shape, got, want, R.rms_norm(x, w, 1e-5, F32), extra=extra)


def test_norm_rows_refuses_unsupported_channels():
    E = _E()
    for C in (100, 320, 1088):          # not a multiple of 64; a multiple without an instantiation; beyond 1024
        out = np.full(2 * C, SENT, F32)
        with pytest.raises(RuntimeError, match="norm_rows"):
            E.test_rowop(2, np.ones(2 * C, F32), 1, 2, C, [np.ones(C, F32)], 1e-5, out, 2 * C)
        assert "norm_rows" in _last_error() and (out == SENT).all()


@pytest.mark.parametrize("T,B", ROW_TB)
@pytest.mark.parametrize("C", [100, 128, 256, 384, 512])
def test_dwconv7_ln(C, T, B, record_property):
    """dwconv7_ln_kernel<1|2>: asymmetric taps, output row t reads rows t .. t + 6, non-zero x_off, batch strides larger than the tensor;
    C = 100 is not a multiple of 64 (the launcher takes multiples of 4)"""
    E = _E()
    rng = np.random.default_rng(C * 1000 + T * 7 + B)
    x_off, xb, ob = 4 * C + 8, (T + 6) * C + 4 * C + 40, T * C + 32
    x = _row_inputs(rng, B, T + 6, C)
    wT = (rng.standard_normal((7, C)) * 0.4 + 0.1 * np.arange(7)[:, None]).astype(F32)          # no two taps alike
    bias, lw, lb = rng.standard_normal(C).astype(F32) * 0.3, rng.uniform(0.5, 1.5, C).astype(F32), rng.standard_normal(C).astype(F32)
    xi, oi = _rows_index(B, T + 6, C, xb, x_off, C), _rows_index(B, T, C, ob, 0, C)
    xflat = _scatter(x, xi, (B - 1) * xb + x_off + (T + 6) * C, fill=1e30)
    out = np.full((B - 1) * ob + T * C + 12, SENT, F32)
    E.test_rowop(0, xflat, B, T, C, [wT, bias, lw, lb], 1e-6, out, xb, x_off, o_bstride=ob)
    shape = "C=%d T=%d B=%d" % (C, T, B)
    written = np.zeros(out.size, bool)
    written[oi.reshape(-1)] = True
    _exact("dwconv7_ln", shape, bool((out[~written] == SENT).all()), "outside the output rows untouched")
    _check(record_property, "dwconv7_ln", shape, out[oi], R.dwconv7_ln(x, wT, bias, lw, lb, 1e-6), R.dwconv7_ln(x, wT, bias, lw, lb, 1e-6, F32))


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("C,T,B", [(128, 10, 2), (384, 43, 3), (512, 4, 64)])
def test_dwconv7_ln_planes_output(C, T, B, n_planes, blocked, record_property):
    E = _E()
    rng = np.random.default_rng(C + T + B + 5)
    x = _row_inputs(rng, B, T + 6, C)
    wT = (rng.standard_normal((7, C)) * 0.4 + 0.1 * np.arange(7)[:, None]).astype(F32)
    bias, lw, lb = rng.standard_normal(C).astype(F32) * 0.3, rng.uniform(0.5, 1.5, C).astype(F32), rng.standard_normal(C).astype(F32)
    out = np.full(B * T * C, SENT, F32)
    _, planes = E.test_rowop(0, x, B, T, C, [wT, bias, lw, lb], 1e-6, out, (T + 6) * C, n_planes=n_planes, blocked=blocked)
    shape = "C=%d T=%d B=%d planes=%d blocked=%d" % (C, T, B, n_planes, blocked)
    _exact("dwconv7_ln planes", shape, bool((out == SENT).all()), "fp32 rows untouched when planes are written")
    got = R.planes_decode(planes, n_planes, B * T, C, blocked).reshape(B, T, C)
    want = R.dwconv7_ln(x, wT, bias, lw, lb, 1e-6)
    extra = (2.0 ** -22 if n_planes == 2 else 2.0 ** -11) * float(np.abs(want).max()) + 2.0 ** -25
    _check(record_property, "dwconv7_ln planes", shape, got, want, R.dwconv7_ln(x, wT, bias, lw, lb, 1e-6, F32), extra=extra)


def test_dwconv7_ln_refuses_unsupported_channels():
    E = _E()
    for C in (768, 130):
        out = np.full(2 * C, SENT, F32)
        with pytest.raises(RuntimeError, match="dwconv7_ln"):
            E.test_rowop(0, np.ones(8 * C, F32), 1, 2, C, [np.ones((7, C), F32)] + [np.ones(C, F32)] * 3, 1e-6, out, 8 * C)
        assert (out == SENT).all()


# =====================================================================================================================================
# BSQ
# =====================================================================================================================================
BSQ_SEEDS = {(1, 1): 0, (10, 2): 1, (43, 3): 34, (3, 64): 24}          # chosen on the CPU so that min |u_fp64| >= 1e-4 (asserted below)


def _bsq_inputs(T, B, seed):
    rng = np.random.default_rng(9000 + 97 * T + B + 1009 * seed)
    C = 512
    z = (rng.standard_normal((B, T, C)) * 2 + 0.1).astype(F32)
    W = (rng.standard_normal((13, C)) / np.sqrt(C) + 0.002 * np.arange(13)[:, None]).astype(F32)
    bias = (rng.standard_normal(13) * 0.1).astype(F32)
    nw = rng.uniform(0.5, 1.5, C).astype(F32)
    return z, W, bias, nw


@pytest.mark.parametrize("zn_on", [False, True])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("T,B", sorted(BSQ_SEEDS))
def test_bsq_indices_exact_and_u(T, B, fused, zn_on, record_property):
    """bsq_kernel: with / without the fused RMSNorm, zn_out on / off, strided rows, idx_bstride / idx_off non-trivial, nbits = 13.  The inputs
    keep every |u_fp64| >= 1e-4 (asserted), so EVERY bit must match -- no element is excluded."""
    E = _E()
    z, W, bias, nw = _bsq_inputs(T, B, BSQ_SEEDS[(T, B)])
    C, ldz, z_off = 512, 512 + 16, 24
    zb, ib, i_off = T * ldz + 40, T + 3, 2
    zi = _rows_index(B, T, C, zb, z_off, ldz)
    zflat = _scatter(z, zi, (B - 1) * zb + z_off + T * ldz, fill=1e30)
    n_idx = (B - 1) * ib + i_off + T + 1
    idx = np.full(n_idx, -5, np.int64)
    u = np.full((n_idx, 13), SENT, F32)
    zn = np.full(zflat.size, SENT, F32) if zn_on else None
    E.test_bsq(zflat, B, T, W, bias, idx, zb, z_off, ldz, norm_w=nw if fused else None, eps=1e-5, zn_out=zn, idx_bstride=ib, idx_off=i_off, u_out=u)
    shape = "T=%d B=%d fused=%d zn=%d" % (T, B, fused, zn_on)
    rows = z.reshape(B * T, C)
    zn64, u64, raw64, idx64 = R.bsq(rows, nw if fused else None, 1e-5, W, bias)
    zn32, u32, _, _ = R.bsq(rows, nw if fused else None, 1e-5, W, bias, F32)
    assert np.abs(u64).min() >= 1e-4, "test inputs must keep every u away from 0 (pick another seed)"
    ii = (np.arange(B)[:, None] * ib + i_off + np.arange(T)[None, :]).reshape(-1)
    _exact("bsq", shape, np.array_equal(idx[ii], idx64), "every index bit")
    rest = np.ones(n_idx, bool)
    rest[ii] = False
    _exact("bsq", shape, bool((idx[rest] == -5).all() and (u[rest] == SENT).all()), "index / u entries outside the rows untouched")
    _check(record_property, "bsq u", shape, u[ii], u64, u32, ceiling=2e-5)
    if zn_on:
        wr = np.zeros(zflat.size, bool)
        if fused:
            wr[zi.reshape(-1)] = True
            _check(record_property, "bsq zn_out", shape, zn[zi].reshape(B * T, C), zn64, zn32)
        _exact("bsq", shape, bool((zn[~wr] == SENT).all()), "zn_out outside the rows untouched")


def test_bsq_without_u_out_and_refusal():
    E = _E()
    z, W, bias, nw = _bsq_inputs(10, 2, BSQ_SEEDS[(10, 2)])
    idx = np.full(20, -5, np.int64)
    E.test_bsq(z, 2, 10, W, bias, idx, 10 * 512, norm_w=nw)
    assert np.array_equal(idx, R.bsq(z.reshape(20, 512), nw, 1e-5, W, bias)[3])
    with pytest.raises(RuntimeError, match="bsq: built for"):
        E.test_bsq(z[..., :256], 2, 10, W[:, :256], bias, idx, 10 * 256)


# =====================================================================================================================================
# STFT ring
# =====================================================================================================================================
STFT_N = 16 * 512
_STFT_REF = {}


def _stft_signals():
    """time-ordered windows [3, N]: silence; three sines off the bin centres + noise; a unit impulse (flat spectrum: a twiddle or
    window-alignment slip cannot average away)"""
    rng = np.random.default_rng(8)
    n = np.arange(STFT_N)
    w = np.zeros((3, STFT_N), F32)
    w[1] = (0.6 * np.sin(2 * np.pi * 100.37 * n / 2048) + 0.3 * np.sin(2 * np.pi * 431.81 * n / 2048 + 1.0) + 0.2 * np.sin(2 * np.pi * 977.5 * n / 2048 + 2.0)
            + 0.05 * rng.standard_normal(STFT_N)).astype(F32)
    w[2, 3 * 512 + 777] = 1.0
    return w


def _stft_ref():
    if not _STFT_REF:
        w = _stft_signals()
        _STFT_REF.update(w=w, f64=R.stft_mag(w), f32=R.stft_mag(w, dt=F32))
    return _STFT_REF["w"], _STFT_REF["f64"], _STFT_REF["f32"]


def _check_stft(record_property, shape, mag, rows_to_frames):
    """mag [B, rows, ldm]; rows_to_frames {output row: window frame}; all other rows keep the sentinel"""
    _, f64, f32 = _stft_ref()
    rows = sorted(rows_to_frames)
    fr = [rows_to_frames[r] for r in rows]
    other = [r for r in range(mag.shape[1]) if r not in rows_to_frames]
    _exact("stft_mag", shape, bool((mag[:, other] == SENT).all()), "rows outside the launch untouched")
    _exact("stft_mag", shape, bool((mag[:, rows, 1025:] == 0.0).all()), "pad columns zero")
    for b, kind in enumerate(("silence", "sines", "impulse")):        # one bound per signal: their scales differ by orders of magnitude
        _check(record_property, "stft_mag " + kind, shape, mag[b, rows, :1025], f64[b, fr], f32[b, fr])
    # silence: sqrt(1e-6) in every bin (1e-3, not 0), to the rounding of the fp32 square root
    assert np.abs(mag[0, rows, :1025].astype(F64) - 1e-3).max() <= 4 * R.ulp32(1e-3)


@pytest.mark.parametrize("n_chunk", [512, 2048, 300])
def test_stft_ring_every_origin(n_chunk, record_property):
    """stft_mag_kernel over every ring origin ((step + add) n_chunk) % N of 1-frame and 4-frame chunks (and one chunk length that is not a
    multiple of the hop: the wrap falls inside a hop), all frames: the frame that spans the ring's end wraps inside itself"""
    E = _E()
    w, _, _ = _stft_ref()
    nfr = STFT_N // 512
    seen = set()
    for step, add in [(s, a) for s in range(0, 40, 3) for a in (0, 1, 5)]:
        origin = ((step + add) * n_chunk) % STFT_N
        if origin in seen or (n_chunk == 300 and len(seen) >= 6):
            continue
        seen.add(origin)
        ring = np.roll(w, origin, axis=1)            # the oldest sample sits at `origin`
        mag = np.full((3, nfr + 2, 1088), SENT, F32)
        E.test_stft_ring(ring, mag, step=step, n_chunk=n_chunk, add=add, m0=0, nfr=nfr)
        _check_stft(record_property, "n_chunk=%d step=%d add=%d origin=%d" % (n_chunk, step, add, origin), mag, {r: r for r in range(nfr)})
    assert len(seen) == (STFT_N // n_chunk if n_chunk != 300 else 6)


def test_stft_ring_ranges_and_null_step(record_property):
    """step == nullptr (origin 0 whatever `add` says), nfr in {1, 4, all}, m0 > 0, and the two-range launch with a gap left at the sentinel"""
    E = _E()
    w, _, _ = _stft_ref()
    nfr = STFT_N // 512
    for m0, n in ((0, 1), (5, 4), (nfr - 1, 1), (0, nfr)):
        mag = np.full((3, nfr + 1, 1088), SENT, F32)
        E.test_stft_ring(w, mag, step=None, n_chunk=2048, add=3, m0=m0, nfr=n)
        _check_stft(record_property, "step=null m0=%d nfr=%d" % (m0, n), mag, {r: m0 + r for r in range(n)})
    origin = (7 + 2) * 2048 % STFT_N
    ring = np.roll(w, origin, axis=1)
    for (m0, n, m0b, nb, rb) in ((0, 3, 12, 4, 9), (2, 1, 15, 1, 1), (0, 6, 6, 10, 8)):
        mag = np.full((3, 20, 1100), SENT, F32)
        E.test_stft_ring(ring, mag, step=7, n_chunk=2048, add=2, m0=m0, nfr=n, second=(m0b, nb, rb))
        rows = {r: m0 + r for r in range(n)}
        rows.update({rb + r: m0b + r for r in range(nb)})
        _check_stft(record_property, "two ranges m0=%d nfr=%d m0b=%d nfrb=%d row_b0=%d" % (m0, n, m0b, nb, rb), mag, rows)
    with pytest.raises(RuntimeError, match="stft: bad shape"):
        E.test_stft_ring(w, np.full((3, 20, 1088), SENT, F32), m0=nfr - 1, nfr=2)


# =====================================================================================================================================
# FSQ, conv_post + tanh
# =====================================================================================================================================
FSQ_SEEDS = {1: 0, 10: 0, 43: 1}          # chosen on the CPU so that every rounding margin is >= 1e-4 (asserted below)


@pytest.mark.parametrize("T", sorted(FSQ_SEEDS))
def test_fsq_encode_indices_exact(T, record_property):
    """fsq_encode_kernel: strided latent rows, strided code layout; every margin of the fp64 evaluation is >= 1e-4 (asserted), so every
    index must match exactly"""
    E = _E()
    B, G, gd = 2, 8, 64
    rng = np.random.default_rng(5000 + T + 131 * FSQ_SEEDS[T])
    x = (rng.standard_normal((B, T, G * gd)) * 1.5).astype(F32)
    Win = (rng.standard_normal((G, 4, gd)) / np.sqrt(gd) + 0.01 * np.arange(4)[None, :, None]).astype(F32)
    bin_ = (rng.standard_normal((G, 4)) * 0.2).astype(F32)
    ld, l_off = G * gd + 64, 128
    lb, cg, cb = T * ld + 200, T + 5, G * (T + 5) + 7
    li = _rows_index(B, T, G * gd, lb, l_off, ld)
    lat = _scatter(x, li, (B - 1) * lb + l_off + T * ld, fill=1e30)
    codes = np.full((B - 1) * cb + (G - 1) * cg + T + 3, -7, np.int32)
    E.test_fsq(True, lat, codes, B, T, G, gd, Win, bin_, lb, l_off, ld, cb, cg)
    want, margin = R.fsq_encode(x, Win, bin_)
    assert margin.min() >= 1e-4, "test inputs must keep every digit away from a rounding boundary (pick another seed)"
    ci = (np.arange(B)[:, None, None] * cb + np.arange(G)[None, :, None] * cg + np.arange(T)[None, None, :])
    shape = "T=%d" % T
    _exact("fsq_encode", shape, np.array_equal(codes[ci], want), "every index")
    rest = np.ones(codes.size, bool)
    rest[ci.reshape(-1)] = False
    _exact("fsq_encode", shape, bool((codes[rest] == -7).all()), "codes outside the layout untouched")


@pytest.mark.parametrize("T", [1, 10, 43])
def test_fsq_decode(T, record_property):
    E = _E()
    B, G, gd = 2, 8, 64
    rng = np.random.default_rng(5100 + T)
    cg, cb = T + 2, G * (T + 2) + 3
    codes_in = rng.integers(0, 1000, (B, G, T)).astype(np.int32)
    codes_in[0, 0, 0], codes_in[-1, -1, -1] = 0, 999
    ci = (np.arange(B)[:, None, None] * cb + np.arange(G)[None, :, None] * cg + np.arange(T)[None, None, :])
    codes = np.zeros((B - 1) * cb + (G - 1) * cg + T, np.int32)
    codes[ci] = codes_in
    Wout = (rng.standard_normal((G, gd, 4)) + 0.1 * np.arange(4)).astype(F32)
    bout = (rng.standard_normal((G, gd)) * 0.1).astype(F32)
    ld, l_off = G * gd + 32, 96
    lb = T * ld + 160
    li = _rows_index(B, T, G * gd, lb, l_off, ld)
    lat = np.full((B - 1) * lb + l_off + T * ld + 9, SENT, F32)
    E.test_fsq(False, lat, codes, B, T, G, gd, Wout, bout, lb, l_off, ld, cb, cg)
    wr = np.zeros(lat.size, bool)
    wr[li.reshape(-1)] = True
    _exact("fsq_decode", "T=%d" % T, bool((lat[~wr] == SENT).all()), "outside the latent rows untouched")
    _check(record_property, "fsq_decode", "T=%d" % T, lat[li], R.fsq_decode(codes_in, Wout, bout), R.fsq_decode(codes_in, Wout, bout, F32))


@pytest.mark.parametrize("T", [1, 10, 43, 300])
def test_conv_post_tanh(T, record_property):
    """conv_post_tanh_kernel (T = 300 crosses its 256-output tile): inputs scaled so that tanh covers the linear region and |y| > 0.999"""
    E = _E()
    B, C, k = 3, 32, 7
    rng = np.random.default_rng(5200 + T)
    x = (rng.standard_normal((B, T + k - 1, C)) * 2 + 0.2).astype(F32)
    w = (rng.standard_normal((k, C)) * 0.12 + 0.01 * np.arange(k)[:, None]).astype(F32)
    x[0, :k] = np.where(w > 0, 6.0, -0.2)          # one output deep in the saturated region whatever T is
    x[-1, T - 1:] *= 0.01                          # and one in the linear region
    bias = np.array([0.03], F32)
    xb, x_off, pb, p_off = (T + k - 1) * C + 24, 2 * C, T + 11, 5
    xi = _rows_index(B, T + k - 1, C, xb, x_off, C)
    xflat = _scatter(x, xi, (B - 1) * xb + x_off + (T + k - 1) * C, fill=1e30)
    pcm = np.full((B - 1) * pb + p_off + T + 4, SENT, F32)
    E.test_conv_post(xflat, pcm, B, T, C, k, w, bias, xb, x_off, pb, p_off)
    pi = (np.arange(B)[:, None] * pb + p_off + np.arange(T)[None, :])
    want = R.conv_post_tanh(x, w, bias)
    assert np.abs(want).max() >= 0.999 and np.abs(want).min() <= 0.1
    rest = np.ones(pcm.size, bool)
    rest[pi.reshape(-1)] = False
    _exact("conv_post_tanh", "T=%d" % T, bool((pcm[rest] == SENT).all()), "outside the pcm rows untouched")
    _check(record_property, "conv_post_tanh", "T=%d" % T, pcm[pi], want, R.conv_post_tanh(x, w, bias, F32))


# =====================================================================================================================================
# the public sva_op_* entry points (include/sva.h) at arbitrary shapes, strides and flags: ONE engine for the whole sweep
# =====================================================================================================================================
class _Ops:
    """device arrays + the raw bindings of prompt_encoders.py on one engine"""

    def __init__(self):
        import ctypes

        import torch
        from oracle import sva_oracle as O
        from streamvoiceanon_amd import engine as E, prompt_encoders as P, specs

        torch.set_grad_enabled(False)
        self.C, self.E = ctypes, E
        self.engine = E.Engine(O.load_synth_weights(0, specs.all_specs()), device=0)       # the smallest weight set an engine is built from
        P._declare(self.engine.lib)
        self.lib, self.h = self.engine.lib, self.engine.h
        self.dev = P._Dev(self.engine)

    def put(self, a):
        return self.dev.put(np.ascontiguousarray(a, F32))

    def get(self, addr, shape):
        return self.dev.get(addr, shape)

    def ok(self, rc, what):
        self.E._check(rc, what)

    def close(self):
        self.dev.free()
        self.engine.close()


@pytest.fixture(scope="module")
def ops():
    o = _Ops()
    yield o
    o.close()


def _strided(rng, T, C, ld, scale=1.0, shift=0.0):
    """[T, ld] rows whose first C columns are data and whose tail is a value that would wreck any result that read it"""
    a = np.full((T, ld), 1e30, F32)
    a[:, :C] = rng.standard_normal((T, C)) * scale + shift + 0.1 * np.arange(C) / C
    return a


@pytest.mark.parametrize("Cin,N,taps,stride,dil,T", [(32, 48, 1, 1, 1, 7), (32, 40, 3, 1, 2, 37), (48, 16, 5, 2, 1, 53), (16, 24, 3, 2, 3, 19), (80, 33, 5, 1, 3, 101),
                                                    (10, 12, 3, 2, 2, 9), (7, 5, 5, 1, 1, 33)])
def test_op_conv(ops, Cin, N, taps, stride, dil, T, record_property):
    """sva_op_conv over stride / dilation / taps with ldx > Cin, ldy > N and T off every block size; Cin % 16 != 0 takes the plain kernel"""
    rng = np.random.default_rng(Cin * 100 + N + taps + stride + dil)
    ldx, ldy = Cin + 12, N + 9
    rows = (T - 1) * stride + (taps - 1) * dil + 1
    x = _strided(rng, rows, Cin, ldx)
    W = (rng.standard_normal((N, taps, Cin)) / np.sqrt(taps * Cin) + 0.01 * np.arange(taps)[None, :, None]).astype(F32)
    bias = rng.standard_normal(N).astype(F32)
    y0 = np.full((T, ldy), SENT, F32)
    dx, dw, db, dy = ops.put(x), ops.put(W), ops.put(bias), ops.put(y0)
    ops.ok(ops.lib.sva_op_conv(ops.h, dx, ldx, T, stride, dil, taps, Cin, dw, db, N, dy, ldy), "sva_op_conv")
    y = ops.get(dy, (T, ldy))
    shape = "Cin=%d N=%d taps=%d stride=%d dil=%d T=%d" % (Cin, N, taps, stride, dil, T)
    _exact("sva_op_conv", shape, bool((y[:, N:] == SENT).all()), "columns beyond N untouched")

    def ref(dt):
        cols = np.concatenate([x[tap * dil:tap * dil + (T - 1) * stride + 1:stride, :Cin] for tap in range(taps)], 1)
        return R._matmul(cols, W.reshape(N, taps * Cin).T, dt) + bias.astype(dt)
    _check(record_property, "sva_op_conv", shape, y[:, :N], ref(F64), ref(F32))


@pytest.mark.parametrize("k,sf,res,relu", [(3, 1, False, True), (3, 2, True, True), (1, 2, False, False), (1, 1, True, False), (3, 2, False, False)])
def test_op_conv2d(ops, k, sf, res, relu, record_property):
    rng = np.random.default_rng(k * 10 + sf + 2 * res + relu)
    Cin, Cout, F, T = 3, 5, 11, 13
    Fo = (F + 2 * (k // 2) - k) // sf + 1
    x = rng.standard_normal((Cin, F, T)).astype(F32)
    W = (rng.standard_normal((Cout, Cin, k, k)) * 0.4 + 0.05 * np.arange(k)[None, None, :, None] - 0.03 * np.arange(k)[None, None, None, :]).astype(F32)
    scale, shift = rng.uniform(0.5, 1.5, Cout).astype(F32), rng.standard_normal(Cout).astype(F32)
    r = rng.standard_normal((Cout, Fo, T)).astype(F32)
    dy = ops.put(np.full((Cout, Fo, T), SENT, F32))
    ops.ok(ops.lib.sva_op_conv2d(ops.h, ops.put(x), Cin, F, T, ops.put(W), Cout, k, sf, ops.put(scale), ops.put(shift), ops.put(r) if res else None, int(relu), dy),
           "sva_op_conv2d")
    y = ops.get(dy, (Cout, Fo, T))

    def ref(dt):
        pad = k // 2
        xp = np.zeros((Cin, F + 2 * pad, T + 2 * pad), dt)
        xp[:, pad:pad + F, pad:pad + T] = x
        acc = np.zeros((Cout, Fo, T), dt)
        for ci in range(Cin):
            for kf in range(k):
                for kt in range(k):
                    acc += W[:, ci, kf, kt].astype(dt)[:, None, None] * xp[ci, kf:kf + (Fo - 1) * sf + 1:sf, kt:kt + T][None]
        acc = acc * scale.astype(dt)[:, None, None] + shift.astype(dt)[:, None, None]
        if res:
            acc = acc + r.astype(dt)
        return np.maximum(acc, 0) if relu else acc
    _check(record_property, "sva_op_conv2d", "k=%d stride_f=%d res=%d relu=%d" % (k, sf, res, relu), y, ref(F64), ref(F32))


@pytest.mark.parametrize("T,C,unbiased", [(1, 100, 0), (2, 100, 1), (2, 64, 0), (37, 100, 1), (301, 70, 0), (301, 192, 1)])
def test_op_colstats(ops, T, C, unbiased, record_property):
    """mean / std over time, biased and unbiased, T = 1 and 2, C not a multiple of 64, ldx > C; entries beyond C untouched"""
    rng = np.random.default_rng(T * 1000 + C + unbiased)
    ld = C + 5
    x = _strided(rng, T, C, ld, scale=2.0, shift=3.0)
    dm, ds = ops.put(np.full(C + 3, SENT, F32)), ops.put(np.full(C + 3, SENT, F32))
    ops.ok(ops.lib.sva_op_colstats(ops.h, ops.put(x), ld, T, C, dm, ds, unbiased), "sva_op_colstats")
    mean, std = ops.get(dm, (C + 3,)), ops.get(ds, (C + 3,))
    shape = "T=%d C=%d unbiased=%d" % (T, C, unbiased)
    _exact("sva_op_colstats", shape, bool((mean[C:] == SENT).all() and (std[C:] == SENT).all()), "entries beyond C untouched")
    xs = x[:, :C]
    m = lambda dt: np.cumsum(xs.astype(dt), axis=0, dtype=dt)[-1] / dt(T)
    s = lambda dt: np.sqrt(np.cumsum((xs.astype(dt) - m(dt)) ** 2, axis=0, dtype=dt)[-1] / dt(T - unbiased))
    _check(record_property, "sva_op_colstats mean", shape, mean[:C], m(F64), m(F32))
    _check(record_property, "sva_op_colstats std", shape, std[:C], s(F64), s(F32))


def test_op_colstats_unbiased_single_row_is_nan_like_torch(ops):
    """torch.std(unbiased=True) of one sample is NaN (0 / 0); so is the kernel's -- documented, not a refusal"""
    import warnings

    import torch
    x = np.arange(1, 9, dtype=F32)[None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # torch warns about the zero degrees of freedom, then returns NaN
        assert torch.isnan(torch.from_numpy(x).std(0, unbiased=True)).all()
    dm, ds = ops.put(np.zeros(8, F32)), ops.put(np.zeros(8, F32))
    ops.ok(ops.lib.sva_op_colstats(ops.h, ops.put(x), 8, 1, 8, dm, ds, 1), "sva_op_colstats")
    assert np.array_equal(ops.get(dm, (8,)), x[0]) and np.isnan(ops.get(ds, (8,))).all()


@pytest.mark.parametrize("T,seg,C", [(250, 100, 128), (7, 100, 70), (200, 100, 64), (101, 25, 96)])
def test_op_cam_context(ops, T, seg, C, record_property):
    """segment mean (the ragged last segment divides by its valid length; seg_len > T: one short segment) + the global mean row"""
    rng = np.random.default_rng(T + seg + C)
    ldy, ldc = C + 4, C + 7
    y = _strided(rng, T, C, ldy, shift=0.5)
    mean = rng.standard_normal(C).astype(F32)
    dc = ops.put(np.full((T, ldc), SENT, F32))
    ops.ok(ops.lib.sva_op_cam_context(ops.h, ops.put(y), ldy, T, C, seg, ops.put(mean), dc, ldc), "sva_op_cam_context")
    ctx = ops.get(dc, (T, ldc))
    shape = "T=%d seg=%d C=%d" % (T, seg, C)
    _exact("sva_op_cam_context", shape, bool((ctx[:, C:] == SENT).all()), "columns beyond C untouched")

    def ref(dt):
        out = np.empty((T, C), dt)
        for lo in range(0, T, seg):
            hi = min(T, lo + seg)
            out[lo:hi] = np.cumsum(y[lo:hi, :C].astype(dt), axis=0, dtype=dt)[-1] / dt(hi - lo) + mean.astype(dt)
        return out
    _check(record_property, "sva_op_cam_context", shape, ctx[:, :C], ref(F64), ref(F32))


@pytest.mark.parametrize("n_valid", [1, 16, 17])
def test_op_attention_valid_keys(ops, n_valid, record_property):
    """Lq queries over the first n_valid of Lk keys; the keys beyond are +-1e4 and must not be seen"""
    rng = np.random.default_rng(n_valid)
    Lq, Lk, H = 5, 17, 3
    D = H * 64
    q = (rng.standard_normal((Lq, D)) * 1.5).astype(F32)
    kv = rng.standard_normal((Lk, 2 * D)).astype(F32)
    kv[:, D:] += 0.25 + 0.1 * np.arange(D) / D
    kv[n_valid:, 0::2], kv[n_valid:, 1::2] = 1e4, -1e4
    do = ops.put(np.full((Lq, D), SENT, F32))
    ops.ok(ops.lib.sva_op_attention(ops.h, ops.put(q), ops.put(kv), Lq, Lk, n_valid, H, do, ops.put(np.zeros((Lq, H, Lk), F32))), "sva_op_attention")
    out = ops.get(do, (Lq, D))
    cache = np.stack([kv[:, :D].reshape(Lk, H, 64).transpose(1, 0, 2), kv[:, D:].reshape(Lk, H, 64).transpose(1, 0, 2)])[None]
    pos, slot = [n_valid - 1] * Lq, [0] * Lq
    _check(record_property, "sva_op_attention", "Lq=%d Lk=%d n_valid=%d" % (Lq, Lk, n_valid), out, R.decode_attention(q, cache, slot, pos, H),
           R.decode_attention(q, cache, slot, pos, H, F32), ceiling=2e-5)
    with pytest.raises(RuntimeError, match="bad key count"):
        ops.ok(ops.lib.sva_op_attention(ops.h, ops.put(q), ops.put(kv), Lq, Lk, Lk + 1, H, do, ops.put(np.zeros((Lq, H, Lk), F32))), "sva_op_attention")


@pytest.mark.parametrize("ldm,sig", [(0, 0), (0, 1), (75, 0), (75, 1)])
def test_op_mul_and_add(ops, ldm, sig, record_property):
    rng = np.random.default_rng(ldm + sig)
    T, C, ldy = 13, 70, 77
    y = _strided(rng, T, C, ldy)
    m = _strided(rng, T if ldm else 1, C, ldm or C, scale=3.0)
    dy = ops.put(y)
    ops.ok(ops.lib.sva_op_mul(ops.h, dy, ldy, ops.put(m), ldm, T, C, sig), "sva_op_mul")
    got = ops.get(dy, (T, ldy))
    shape = "ldm=%d sigmoid=%d" % (ldm, sig)
    _exact("sva_op_mul", shape, np.array_equal(got[:, C:], y[:, C:]), "columns beyond C untouched")
    ref = lambda dt: y[:, :C].astype(dt) * ((dt(1) / (dt(1) + np.exp(-m[:, :C].astype(dt)))) if sig else m[:, :C].astype(dt))
    _check(record_property, "sva_op_mul", shape, got[:, :C], ref(F64), ref(F32))
    ops.ok(ops.lib.sva_op_add(ops.h, dy, ldy, ops.put(y), ldy, T, C), "sva_op_add")
    got2 = ops.get(dy, (T, ldy))
    _exact("sva_op_add", shape, np.array_equal(got2[:, :C], got[:, :C] + y[:, :C]) and np.array_equal(got2[:, C:], y[:, C:]), "one fp32 addition, columns beyond C untouched")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_op_affine_relu_modes(ops, mode, record_property):
    rng = np.random.default_rng(mode)
    T, C, ldx, ldy = 11, 70, 73, 79
    x = _strided(rng, T, C, ldx)
    scale, shift = (rng.standard_normal(C) + 0.2).astype(F32), rng.standard_normal(C).astype(F32)       # negative scales: the two ReLU placements differ
    for sc, sh in ((scale, shift), (None, shift), (scale, None)):
        dy = ops.put(np.full((T, ldy), SENT, F32))
        ops.ok(ops.lib.sva_op_affine(ops.h, ops.put(x), ldx, T, C, None if sc is None else ops.put(sc), None if sh is None else ops.put(sh), mode, dy, ldy), "sva_op_affine")
        y = ops.get(dy, (T, ldy))
        shape = "mode=%d scale=%d shift=%d" % (mode, sc is not None, sh is not None)
        _exact("sva_op_affine", shape, bool((y[:, C:] == SENT).all()), "columns beyond C untouched")

        def ref(dt):
            v = x[:, :C].astype(dt)
            v = np.maximum(v, 0) if mode == 2 else v
            v = v * (dt(1) if sc is None else sc.astype(dt)) + (dt(0) if sh is None else sh.astype(dt))
            return np.maximum(v, 0) if mode == 1 else v
        _check(record_property, "sva_op_affine", shape, y[:, :C], ref(F64), ref(F32))


def test_op_unary(ops, record_property):
    """ops 1 - 4: log(max(x, p0)) with x <= 0, the level-4 FSQ quantiser away from its rounding boundaries, sigmoid, negate"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(1003) * 3).astype(F32)
    x[:4] = [0.0, -1.0, 1e-12, -0.0]
    p0 = float(np.finfo(F32).eps)
    half_l = 3 * (1 + 1e-3) / 2
    bounded = lambda v: np.tanh(v.astype(F64) + np.arctanh(0.5 / half_l)) * half_l - 0.5
    xq = x[np.abs(bounded(x) - np.rint(bounded(x))) < 0.5 - 1e-4]          # margin rule as for fsq_encode: asserted non-trivial below
    assert xq.size > 900
    refs = {1: lambda v, dt: np.log(np.maximum(v.astype(dt), dt(p0))), 3: lambda v, dt: dt(1) / (dt(1) + np.exp(-v.astype(dt))), 4: lambda v, dt: -v.astype(dt)}
    for op in (1, 3, 4):
        d = ops.put(np.concatenate([x, [SENT]]))
        ops.ok(ops.lib.sva_op_unary(ops.h, d, x.size, op, p0), "sva_op_unary")
        got = ops.get(d, (x.size + 1,))
        _exact("sva_op_unary", "op=%d" % op, bool(got[-1] == SENT), "element beyond n untouched")
        _check(record_property, "sva_op_unary", "op=%d n=%d" % (op, x.size), got[:-1], refs[op](x, F64), refs[op](x, F32))
    d = ops.put(xq)
    ops.ok(ops.lib.sva_op_unary(ops.h, d, xq.size, 2, 0.0), "sva_op_unary")
    _exact("sva_op_unary", "op=2 n=%d" % xq.size, np.array_equal(ops.get(d, (xq.size,)), (np.rint(bounded(xq)) / 2).astype(F32)), "every level exact")


@pytest.mark.parametrize("Dh,T", [(341, 32), (7, 3), (64, 5)])
def test_op_geglu(ops, Dh, T, record_property):
    """odd Dh (341 is the product's): out = gelu(h[:, Dh:2 Dh]) * h[:, :Dh], pad columns Dh .. ldo zero"""
    from math import erf
    rng = np.random.default_rng(Dh)
    ldh, ldo = 2 * Dh + 6, Dh + 11
    h = _strided(rng, T, 2 * Dh, ldh, scale=2.0)
    do = ops.put(np.full((T, ldo), SENT, F32))
    ops.ok(ops.lib.sva_op_geglu(ops.h, ops.put(h), ldh, T, Dh, do, ldo), "sva_op_geglu")
    out = ops.get(do, (T, ldo))
    _exact("sva_op_geglu", "Dh=%d T=%d" % (Dh, T), bool((out[:, Dh:] == 0.0).all()), "pad columns zero")
    verf = np.vectorize(erf)

    def ref(dt):
        g, a = h[:, Dh:2 * Dh].astype(dt), h[:, :Dh].astype(dt)
        return (dt(0.5) * g * (dt(1) + verf(g.astype(F64) * 0.7071067811865476).astype(dt)) * a).astype(dt)
    _check(record_property, "sva_op_geglu", "Dh=%d T=%d" % (Dh, T), out[:, :Dh], ref(F64), ref(F32))


def test_op_l2norm_near_zero_row(ops, record_property):
    """F.normalize(x) * scale * gamma with its 1e-12 floor: a zero row stays zero (no NaN), a 1e-20 row is scaled by 1e12, not normalised"""
    rng = np.random.default_rng(12)
    T, C = 6, 128
    x = rng.standard_normal((T, C)).astype(F32)
    x[1] = 0.0
    x[2] *= 1e-20
    x[3] *= 1e-6
    x[4] *= 1e4
    gamma = rng.uniform(0.5, 1.5, C).astype(F32)
    dy = ops.put(np.full((T, C), SENT, F32))
    ops.ok(ops.lib.sva_op_l2norm(ops.h, ops.put(x), T, C, ops.put(gamma), float(C ** 0.5), dy), "sva_op_l2norm")
    y = ops.get(dy, (T, C))

    def ref(dt):
        v = x.astype(dt)
        n = np.sqrt(R._sum(v * v, dt))
        return v * (dt(C ** 0.5) / np.maximum(n, dt(1e-12)))[:, None] * gamma.astype(dt)
    assert (y[1] == 0).all()
    _check(record_property, "sva_op_l2norm", "T=%d C=%d" % (T, C), y, ref(F64), ref(F32))


def _dft_mag(frames, dt, power):
    n = frames.shape[1]
    ang = np.remainder(np.outer(np.arange(n), np.arange(n // 2 + 1)), n) * (2.0 * np.pi / n)
    re, im = R._matmul(frames.astype(dt), np.cos(ang).astype(dt), dt), R._matmul(frames.astype(dt), (-np.sin(ang)).astype(dt), dt)
    p = re * re + im * im
    return p if power else np.sqrt(p)


@pytest.mark.parametrize("n", [600, 1023, 3207])
def test_op_stft_mag_short_and_ragged(ops, n, record_property):
    """torch.stft(center=True, reflect) magnitude with a 640-sample periodic Hann centred in 1024: a wave shorter than one frame (600, 1023)
    and n not a multiple of the hop; frames_out = 1 + n // hop; pad columns zero"""
    rng = np.random.default_rng(n)
    n_fft, win, hop, ldo = 1024, 640, 320, 528
    wave = (np.sin(2 * np.pi * 0.0371 * np.arange(n)) * 0.5 + 0.1 * rng.standard_normal(n)).astype(F32)
    m = 1 + n // hop
    mo = ops.C.c_int(0)
    dsp = ops.put(np.full((m + 1, ldo), SENT, F32))
    ops.ok(ops.lib.sva_op_stft_mag(ops.h, ops.put(wave), n, n_fft, win, hop, ops.put(np.zeros((m, n_fft), F32)), dsp, ldo, ops.C.byref(mo)), "sva_op_stft_mag")
    spec = ops.get(dsp, (m + 1, ldo))
    assert mo.value == m
    _exact("sva_op_stft_mag", "n=%d" % n, bool((spec[:m, 513:] == 0).all() and (spec[m] == SENT).all()), "pad columns zero, no frame beyond frames_out")

    def ref(dt):
        w = np.zeros(n_fft, dt)
        w[(n_fft - win) // 2:(n_fft + win) // 2] = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)).astype(dt)
        y = np.pad(wave.astype(dt), n_fft // 2, mode="reflect")
        return _dft_mag(np.stack([y[i * hop:i * hop + n_fft] for i in range(m)]) * w, dt, False)
    _check(record_property, "sva_op_stft_mag", "n=%d frames=%d" % (n, m), spec[:m, :513], ref(F64), ref(F32))
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        ops.ok(ops.lib.sva_op_stft_mag(ops.h, ops.put(wave), 512, n_fft, win, hop, ops.put(np.zeros((m, n_fft), F32)), dsp, ldo, ops.C.byref(mo)), "sva_op_stft_mag")


@pytest.mark.parametrize("n", [400, 559, 1771])
def test_op_fbank_power_short_and_ragged(ops, n, record_property):
    """Kaldi fbank power spectrum (snip_edges, DC removal, pre-emphasis 0.97, povey window, 512-point DFT): exactly one frame (400), n not
    a multiple of the 160-sample shift; a wave shorter than one frame is refused"""
    rng = np.random.default_rng(n)
    ldo = 272
    wave = ((np.sin(2 * np.pi * 0.0513 * np.arange(n)) * 0.4 + 0.1 * rng.standard_normal(n) + 0.05) * 32768).astype(F32)
    m = 1 + (n - 400) // 160
    mo = ops.C.c_int(0)
    dsp = ops.put(np.full((m + 1, ldo), SENT, F32))
    ops.ok(ops.lib.sva_op_fbank_power(ops.h, ops.put(wave), n, ops.put(np.zeros((m, 512), F32)), dsp, ldo, ops.C.byref(mo)), "sva_op_fbank_power")
    spec = ops.get(dsp, (m + 1, ldo))
    assert mo.value == m
    _exact("sva_op_fbank_power", "n=%d" % n, bool((spec[:m, 257:] == 0).all() and (spec[m] == SENT).all()), "pad columns zero, no frame beyond frames_out")

    def ref(dt):
        fr = np.stack([wave[i * 160:i * 160 + 400] for i in range(m)]).astype(dt)
        fr = fr - (R._sum(fr, dt) / dt(400))[:, None]
        fr = fr - dt(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], 1)
        w = ((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)) ** 0.85).astype(dt)
        return _dft_mag(np.concatenate([fr * w, np.zeros((m, 112), dt)], 1), dt, True)
    _check(record_property, "sva_op_fbank_power", "n=%d frames=%d" % (n, m), spec[:m, :257], ref(F64), ref(F32))
    with pytest.raises(RuntimeError, match="shorter than one 25 ms frame"):
        ops.ok(ops.lib.sva_op_fbank_power(ops.h, ops.put(wave), 399, ops.put(np.zeros((m, 512), F32)), dsp, ldo, ops.C.byref(mo)), "sva_op_fbank_power")


def test_op_cf_to_rows(ops):
    rng = np.random.default_rng(4)
    CF, T, ldy = 37, 11, 41
    x = rng.standard_normal((CF, T)).astype(F32)
    dy = ops.put(np.full((T, ldy), SENT, F32))
    ops.ok(ops.lib.sva_op_cf_to_rows(ops.h, ops.put(x), CF, T, dy, ldy), "sva_op_cf_to_rows")
    y = ops.get(dy, (T, ldy))
    assert np.array_equal(y[:, :CF], x.T) and (y[:, CF:] == SENT).all()
