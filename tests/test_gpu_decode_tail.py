"""The tail of the AR decode, kernel by kernel, against the references of tests/kernel_refs.py: the samplers that run by default
(launch_sampler, launch_sampler_small and the four ardev::nucleus_sample instantiations of the persistent kernels), launch_gemv in its
plain and SwiGLU modes, ardev::gemv over float and fp16 weight fragments, the logit edits and the token / history kernels -- through the
hooks sva_test_sampler_launch, sva_test_ar_device, sva_test_gemv and sva_test_token_ops (csrc/testhooks.hip).

Tokens are compared EXACTLY with kernel_refs.nucleus_token (float64).  That is sound because every row these tests use is decidable --
float32 rounding inside a kernel cannot change its winner -- which test_kernel_refs.py asserts on the CPU over the same generators
(decode_tail_cases.py).  Floating results use the one derived bound of test_gpu_kernels.py, 4 e32 + 4 ulp32(max |ref|); copies, edits
(one float32 multiply or divide) and in-order float32 sums are exact.  Every refusal is a host-side check: nothing is launched.

With SVA_DECODE_TAIL_PARITY_TABLE=<path> the run writes its table there (profiles/decode_tail_parity.txt)."""
import os
import time

import numpy as np
import pytest

import decode_tail_cases as G
import kernel_refs as R
import test_gpu_kernels as K

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = 777.0
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    t0 = time.time()
    yield
    path = os.environ.get("SVA_DECODE_TAIL_PARITY_TABLE")
    if path and _TABLE:
        floats = [t for t in _TABLE if not t[2]]
        with open(path, "w") as f:
            f.write("# %d cases (%d compared with float64, %d exact checks), worst err / bound = %.3f, wall %.1f s\n" %
                    (len(_TABLE), len(floats), len(_TABLE) - len(floats), max(t[5] for t in _TABLE), time.time() - t0))
            f.write("%-26s %-72s %12s %12s %8s\n" % ("kernel", "shape", "max_err", "bound", "ratio"))
            for k, s, what, e, b, r in floats:
                f.write("%-26s %-72s %12.4e %12.4e %8.3f\n" % (k, s, e, b, r))
            # the exact checks, one row per (kernel, property): how many cases held it, how many did not
            f.write("\n%-26s %-92s %6s %6s\n" % ("kernel", "exact property", "held", "failed"))
            rows = {}
            for k, s, what, e, b, r in _TABLE:
                if what:
                    c = rows.setdefault((k, what.split(" (first differing")[0]), [0, 0])
                    c[0 if r == 0.0 else 1] += 1
            for (k, what), (ok, bad) in rows.items():
                f.write("%-26s %-92s %6d %6d\n" % (k, what, ok, bad))


def _mine(fn, kernel, tag, exact, *a, **kw):
    """the comparison helpers of test_gpu_kernels.py, their table rows moved into this module's table"""
    n = len(K._TABLE)
    try:
        return fn(*a, **kw)
    finally:
        _TABLE.extend((kernel, str(tag), exact, e, b, r) for (_, _, e, b, r) in K._TABLE[n:])
        del K._TABLE[n:]


def _check(record_property, kernel, tag, *a, **kw):
    return _mine(K._check, kernel, tag, "", record_property, kernel, tag, *a, **kw)


def _exact(kernel, tag, ok, what):
    return _mine(K._exact, kernel, tag, what, kernel, tag, ok, what)


def _E():
    from streamvoiceanon_amd import engine as E
    return E


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# =====================================================================================================================================
# samplers
# =====================================================================================================================================
def _want(L, Q, tp, temp):
    return np.array([R.nucleus_token(L[r], Q[r], temp, tp)[0] for r in range(L.shape[0])], np.int32)


def _launch_plain(small, L, Q, tp, temp, **kw):
    """launch_sampler / launch_sampler_small on dense rows; host noise Q [rows, V] (None: device RNG, seed / frame in kw)"""
    rows, V = L.shape
    tok_raw = np.full(rows, -7, np.int32)
    tok = np.full(rows, -7, np.int32) if small else None
    _E().test_sampler_launch(L.reshape(-1).copy(), rows, V, V, small=small, noise=None if Q is None else Q.reshape(-1), ldn=V, temperature=temp, top_p=tp,
                             tok_raw=tok_raw, tok=tok, **kw)
    if small:
        assert np.array_equal(tok, tok_raw)                    # no forcing: tok = the sample
    return tok_raw


def _impls(V):
    """name -> callable(L, Q, tp, temp, **rng) -> (tokens, every-thread flag or None) for every implementation that takes this V"""
    E = _E()
    out = {}
    if V <= 8192:
        for inst, (nw, per, vmax) in E.AR_NUCLEUS_INSTS.items():
            if V <= vmax:
                out["nucleus_sample<%d,%d>" % (nw, per)] = (lambda L, Q, tp, temp, inst=inst, **kw: E.test_ar_nucleus(inst, L, Q, temperature=temp, top_p=tp, **kw))
    if V <= 1024:
        out["launch_sampler_small"] = lambda L, Q, tp, temp, **kw: (_launch_plain(True, L, Q, tp, temp, **kw), None)
    out["launch_sampler"] = lambda L, Q, tp, temp, **kw: (_launch_plain(False, L, Q, tp, temp, **kw), None)
    return out


def _compare_all(V, tag, L, Q, settings, also_variant1=False):
    E = _E()
    impls = _impls(V)
    assert len(impls) >= (1 if V in G.V_SORT else 3)
    for tp, temp in settings:
        want = _want(L, Q, tp, temp)
        base = E.test_sampler(L, Q, 1, temperature=temp, top_p=tp) if also_variant1 else None
        for name, fn in impls.items():
            got, same = fn(L, Q, tp, temp)
            shape = "%s V=%d top_p=%g T=%g" % (tag, V, tp, temp)
            _exact(name, shape, bool((got == want).all()), "tokens == nucleus_token (first differing rows %s)" % np.nonzero(got != want)[0][:6])
            if base is not None:
                _exact(name, shape, bool((got == base).all()), "tokens == the sorting kernel (variant 1)")
            if same is not None:
                _exact(name, shape, bool(same.all()), "every participating thread returned the token")


@pytest.mark.parametrize("V", G.V_ALL)
def test_samplers_random_rows(V):
    """16 rows of the existing sampler test's generator at five (top_p, temperature) settings: V = 1 and 63 (most lanes idle), 1000 / 4097 /
    8191 (ragged last slot), 1024 / 8192 (full), 2048 / 8193 (launch_sampler's LDS sort, P = 2048 and 16384 of dynamic LDS)"""
    L, Q = G.random_rows(V)
    _compare_all(V, "random", L[:G.RANDOM_ROWS], Q[:G.RANDOM_ROWS], G.RANDOM_SETTINGS)


@pytest.mark.parametrize("V", G.V_ALL)
def test_samplers_hard_rows(V):
    """decode_tail_cases.hard_rows: ties, uniform, underflow, -inf, a one-token nucleus, the keep-all branch, the cut inside a tie class on
    the last ids -- exact against float64 AND against the sorting kernel, whose tie rule (smaller id first) is the contract"""
    T, Q = G.hard_rows(V)
    _compare_all(V, "hard", T, Q, G.HARD_SETTINGS, also_variant1=True)


@pytest.mark.parametrize("V", sorted(G.RNG_SEEDS))
def test_sampler_device_rng_equals_host_twin(V):
    """noise = nullptr: the counter RNG keyed by (seed[row], frame[row], kind) at element noise_elem_off + e.  The token equals the same call
    fed synth_weights.exp1_noise(seed, frame, kind, off + V)[off:] -- per-row distinct seeds and frames, kind 0 / 1, off = cb V for cb 0 / 7"""
    for kind in (0, 1):
        for cb in (0, 7):
            L, Q, seed, frame, off = G.rng_case(V, kind, cb)
            want = _want(L, Q, 0.7, 0.7)
            for name, fn in _impls(V).items():
                fed, _ = fn(L, Q, 0.7, 0.7)
                dev, same = fn(L, None, 0.7, 0.7, seed=seed, frame=frame, kind=kind, noise_elem_off=off)
                shape = "V=%d kind=%d noise_elem_off=%d" % (V, kind, off)
                _exact(name, shape, bool((dev == fed).all() and (dev == want).all()), "device RNG == host noise == nucleus_token")
                if same is not None:
                    _exact(name, shape, bool(same.all()), "every participating thread returned the token")


@pytest.mark.parametrize("use_forced", [0, 1])
def test_sampler_small_production_form(use_forced):
    """launch_sampler_small as stages.hip calls it for codebook 5 of [B = 3][8][1000] logits: ldl = 8000 behind a column offset, the noise row of a
    step, tok_stride = 8, forced codes at stride 8 chunk, the fast_emb gather fused"""
    E = _E()
    p = G.PROD
    B, ncb, cbs, cb, chunk, D, ci = p["B"], p["ncb"], p["cbs"], p["cb"], p["chunk"], p["D"], 1
    L, Q = G.production_case()
    Lr, Qr = G.production_rows()
    want = _want(Lr, Qr, 0.7, 0.7)
    rng = np.random.default_rng(31)
    emb = rng.standard_normal((cbs, D)).astype(F32)
    forced = rng.integers(0, cbs, (B, ncb, chunk)).astype(np.int32)
    ldo = D + 8
    for with_table in (True, False):
        logits = L.reshape(-1).copy()
        tok_raw, tok = np.full(B * ncb, -7, np.int32), np.full(B * ncb, -7, np.int32)
        emb_out = np.full(B * ldo, SENT, F32)
        E.test_sampler_launch(logits, B, cbs, ncb * cbs, col_off=cb * cbs, small=True, noise=Q.reshape(-1), ldn=Q.shape[1], noise_off=p["vocab"] + cb * cbs,
                              kind=1, noise_elem_off=cb * cbs, temperature=0.7, top_p=0.7, tok_raw=tok_raw, tok=tok, tok_stride=ncb, tok_off=cb,
                              forced=forced.reshape(-1), forced_stride=ncb * chunk, forced_off=cb * chunk + ci, use_forced=use_forced,
                              emb_table=emb if with_table else None, emb_out=emb_out, ldo=ldo)
        shape = "use_forced=%d table=%d" % (use_forced, with_table)
        raw, tk = tok_raw.reshape(B, ncb), tok.reshape(B, ncb)
        _exact("launch_sampler_small", shape, bool((raw[:, cb] == want).all()), "tok_raw is the sample")
        final = forced[:, cb, ci] if use_forced else want
        _exact("launch_sampler_small", shape, bool((tk[:, cb] == final).all()), "tok is the forced code when forcing is on, else the sample")
        rest = np.ones(ncb, bool)
        rest[cb] = False
        _exact("launch_sampler_small", shape, bool((raw[:, rest] == -7).all() and (tk[:, rest] == -7).all()), "the other codebooks' tokens untouched")
        _exact("launch_sampler_small", shape, bool(np.array_equal(_bits(logits), _bits(L.reshape(-1)))), "logits untouched")
        eo = emb_out.reshape(B, ldo)
        if with_table:
            _exact("launch_sampler_small", shape, bool(np.array_equal(_bits(eo[:, :D]), _bits(emb[final]))), "emb_out == fast_emb[tok] bit for bit")
            _exact("launch_sampler_small", shape, bool((eo[:, D:] == SENT).all()), "emb_out pad untouched")
        else:
            _exact("launch_sampler_small", shape, bool((emb_out == SENT).all()), "no table: nothing written to emb_out")


@pytest.mark.parametrize("V", sorted(G.EDIT_SEEDS))
def test_logit_edits_then_sampler(V):
    """launch_logit_edits, then the sampler, on the same device rows as stages.hip runs them: prev with duplicates, -1 entries and an id >= V; a
    suppress list for the token head.  The edited rows equal the float32 restatement bit for bit; the token equals the oracle's sample_token
    with the same edits (the entries the kernel skips removed: the oracle cannot index them) and nucleus_token on the edited rows"""
    import torch
    from oracle import sva_oracle as O
    L, Q, prev, sup = G.edits_case(V)
    rows = L.shape[0]
    edited, _ = G.edited_rows(V)
    ok_prev = torch.from_numpy(prev[(prev >= 0) & (prev < V)].astype(np.int64))
    ok_sup = [int(s) for s in sup if 0 <= s < V]
    want = np.array([O.sample_token(torch.from_numpy(L[r]), torch.from_numpy(Q[r]), 0.7, 0.7, ok_prev, G.EDIT_PENALTY, ok_sup or None) for r in range(rows)])
    assert (want == _want(edited, Q, 0.7, 0.7)).all()
    assert (want != _want(L, Q, 0.7, 0.7)).any()                  # the edits matter: without them another token wins
    for small in ([True, False] if V <= 1024 else [False]):
        name = "launch_sampler_small" if small else "launch_sampler"
        ldl = V + 8
        logits = np.full(rows * ldl, SENT, F32)
        logits.reshape(rows, ldl)[:, :V] = L
        tok_raw = np.full(rows, -7, np.int32)
        _E().test_sampler_launch(logits, rows, V, ldl, small=small, noise=Q.reshape(-1), ldn=V, temperature=0.7, top_p=0.7, tok_raw=tok_raw,
                                 tok=np.full(rows, -7, np.int32) if small else None, edits=dict(prev=prev, suppress=sup, penalty=G.EDIT_PENALTY, prev_cap=4096))
        got = logits.reshape(rows, ldl)
        _exact(name, "edits V=%d" % V, bool(np.array_equal(_bits(got[:, :V]), _bits(edited)) and (got[:, V:] == SENT).all()), "edited rows == float32 restatement, pad untouched")
        _exact(name, "edits V=%d" % V, bool((tok_raw == want).all()), "token == oracle sample_token with the same edits")


def test_logit_edits_alone():
    """launch_logit_edits: W = 0 / 1 / 4096 = prev_cap / beyond prev_cap (clamped), duplicates (each listed token once, from the original score),
    positive / negative / zero / -inf scores, ldl > V with a sentinel in the pad, suppress ids negative and >= V (ignored), prev_cap = 4097 refused"""
    E = _E()
    rng = np.random.default_rng(41)
    V, rows = 8192, 2
    ldl = V + 8
    base = (rng.standard_normal((rows, V)) * 3).astype(F32)
    base[:, 10] = 0.0
    base[:, 11] = -0.0
    base[:, 12] = -np.inf
    base[:, 13] = -2.5
    base[:, 14] = 3.0
    many = rng.integers(0, V, 5000).astype(np.int32)
    many[4096:] = np.setdiff1d(np.arange(V), many[:4096])[:904]            # ids behind the cap that the first 4096 do not list
    cases = [("W=0", np.zeros(0, np.int32), None, [5, 6]), ("W=1", np.array([14], np.int32), None, []), ("W=1 neg", np.array([13], np.int32), None, []),
             ("dups", np.array([3, 3, 11, 3, 10, 12, -1, V, V + 9, 4], np.int32), None, [-1, V, V + 5, 7]), ("W=4096", many[:4096], None, [1]),
             ("W=5000>cap", many, 5000, []), ("W=3 of 10", np.array([3, 4, 5, 6, 7, 8, 9, 13, 14, 15], np.int32), 3, [])]
    for tag, prev, W, sup in cases:
        logits = np.full(rows * ldl, SENT, F32)
        logits.reshape(rows, ldl)[:, :V] = base
        E.test_logit_edits(logits, rows, V, ldl, prev, sup, 1.5, W=W)
        got = logits.reshape(rows, ldl)
        want = np.stack([R.logit_edits(base[r], prev, sup, 1.5, W=W) for r in range(rows)])
        if tag != "W=0":
            assert not np.array_equal(_bits(want), _bits(base))
        _exact("launch_logit_edits", tag, bool(np.array_equal(_bits(got[:, :V]), _bits(want))), "rows == float32 restatement bit for bit")
        _exact("launch_logit_edits", tag, bool((got[:, V:] == SENT).all()), "pad behind V untouched")
    logits = base.reshape(-1).copy()
    with pytest.raises(E.Refused, match="logit edits: at most 4096"):
        E.test_logit_edits(logits, rows, V, V, many[:4097], [], 1.5, prev_cap=4097)
    _exact("launch_logit_edits", "prev_cap=4097", bool(np.array_equal(_bits(logits), _bits(base.reshape(-1)))), "refused: nothing launched")


# =====================================================================================================================================
# launch_gemv, modes 0 and 1
# =====================================================================================================================================
#            M, K,    N,    mode, norm, bias, res,     ldy,  y_off, ldx pad, scaled rows
GEMV_CASES = [(1, 768, 4, 0, True, True, None, None, 0, 0, False),                 # one unit, three idle waves
              (2, 768, 1000, 0, True, False, None, 8000, 5000, 0, True),           # the fused codebook head: [B][8][1000] behind a column offset
              (3, 768, 768, 0, False, True, "res", None, 0, 8, True),              # MR = 4 at M = 3; bias + residual; ldx > K
              (4, 768, 768, 0, False, False, "alias", 776, 0, 0, True),            # wo as ar_layers_pass runs it: res == Y
              (2, 768, 8192, 0, True, False, None, None, 0, 0, False),             # the fused token head
              (3, 768, 8192, 0, True, True, None, None, 0, 4, False),
              (1, 2304, 768, 0, False, True, "res", None, 0, 0, False),
              (2, 2304, 768, 0, False, False, "alias", None, 0, 4, True),          # w2 + residual in place
              (4, 2304, 768, 0, False, False, "alias", 772, 0, 0, True),
              (3, 2304, 4, 0, True, False, None, None, 0, 0, False),
              (1, 768, 64, 1, True, False, None, None, 0, 0, False),               # SwiGLU: one 32-row group pair
              (2, 768, 4608, 1, True, False, None, None, 0, 0, True),              # w1 | w3 of the AR layers
              (4, 768, 4608, 1, True, False, None, 2312, 0, 8, True),
              (3, 2304, 64, 1, False, False, None, None, 0, 0, False)]


@pytest.mark.parametrize("case", GEMV_CASES, ids=lambda c: "M%d-K%d-N%d-mode%d" % c[:4])
def test_gemv_plain_and_swiglu(case, record_property):
    M, Kd, N, mode, norm, has_bias, res_kind, ldy, y_off, pad, scaled = case
    rng = np.random.default_rng(sum(case[:4]) + 97)
    n_out = N // 2 if mode == 1 else N
    ldx, ldy = Kd + pad, n_out if ldy is None else ldy
    W = (rng.standard_normal((N, Kd)) / np.sqrt(Kd)).astype(F32)
    x = rng.standard_normal((M, Kd)).astype(F32)
    if scaled:
        x[0] *= 1e4
        x[-1] *= 1e-4
    nw = rng.uniform(0.5, 1.5, Kd).astype(F32) if norm else None
    bias = (rng.standard_normal(N) * 0.5).astype(F32) if has_bias else None
    res = rng.standard_normal((M, N)).astype(F32) if res_kind else None
    X = np.full((M, ldx), 1e30, F32)
    X[:, :Kd] = x
    Y = np.full(y_off + (M - 1) * ldy + n_out + 5, SENT, F32)
    cols = y_off + np.arange(M)[:, None] * ldy + np.arange(n_out)[None, :]
    if res_kind == "alias":
        Y[cols] = res
    _E().test_gemv(W, Y, M, N, Kd, X=X, ldx=ldx, ldy=ldy, y_off=y_off, norm_w=nw, bias=bias, res=res if res_kind == "res" else None, ldr=N if res_kind == "res" else ldy,
                   alias=res_kind == "alias", mode=mode)
    kw = dict(norm_w=nw, eps=1e-5, bias=bias, res=res, swiglu=mode == 1)
    name = "launch_gemv mode %d" % mode
    shape = "M=%d K=%d N=%d%s%s%s ldy=%d+%d ldx=%d%s" % (M, Kd, N, " norm" if norm else "", " bias" if has_bias else "", " " + res_kind if res_kind else "", ldy, y_off, ldx,
                                                          " rows x1e4/x1e-4" if scaled else "")
    rest = np.ones(Y.size, bool)
    rest[cols.reshape(-1)] = False
    _exact(name, shape, bool((Y[rest] == SENT).all()), "outside the stored columns untouched")
    _check(record_property, name, shape, Y[cols], R.gemv_ref(x, W, **kw), R.gemv_ref(x, W, dt=F32, **kw))


def test_gemv_refusals_come_from_the_launcher():
    """launch_gemv's own checks, reached through a hook that checks array lengths only: M = 0 / 5, K = 512, ldx % 4, the attention modes with M = 3,
    S = 9 or a norm weight, and SwiGLU with N % 32 != 0 (its last features would read weight rows past W).  Nothing is launched: Y keeps its fill."""
    E = _E()
    rng = np.random.default_rng(5)
    W = rng.standard_normal((768, 768)).astype(F32)
    X = rng.standard_normal((5, 772)).astype(F32)
    nw = np.ones(768, F32)

    def refused(what, match, **kw):
        Y = np.full(5 * 768, SENT, F32)
        args = dict(M=2, N=768, K=768, X=X, ldx=772, mode=0)
        args.update(kw)
        with pytest.raises(E.Refused, match=match):
            E.test_gemv(args.pop("W", W), Y, **args)
        _exact("launch_gemv", what, bool((Y == SENT).all()), "refused by launch_gemv: nothing launched")

    refused("M=0", "gemv: M must be 1..4", M=0)
    refused("M=5", "gemv: M must be 1..4", M=5)
    refused("K=512", "gemv: unsupported K", K=512, W=W[:, :512].copy())
    refused("ldx=770", "gemv: K must be a multiple of 256", ldx=770, X=X.reshape(-1)[:5 * 770].copy())
    for mode, msg in ((3, "gemv: fused attention needs"), (4, "gemv: partial merge needs")):
        refused("mode %d M=3" % mode, msg, mode=mode, M=3, X=None, S=8, H=12)
        refused("mode %d S=9" % mode, msg, mode=mode, X=None, S=9, H=12)
        refused("mode %d norm_w" % mode, msg, mode=mode, X=None, S=8, H=12, norm_w=nw)
    refused("mode 1 N=48", "gemv: SwiGLU needs N", mode=1, N=48, W=W[:64].copy())            # (64 rows given: the hook's length check passes)
    refused("mode 1 N=80", "gemv: SwiGLU needs N", mode=1, N=80, W=W[:128].copy())


# =====================================================================================================================================
# ardev::gemv over WFrag<float> / WFrag<__half>
# =====================================================================================================================================
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("inst", range(10))
def test_ardev_gemv_instantiations(inst, half, record_property):
    """the ten instantiations of ar_decode.hip / ar_batch.hip, three groups of ROWS rows each: one weight row has its last four elements (the
    fp16 fragment's tail) as its only non-zeros; M = 2: one input row scaled by 1e4, one by 1e-4; ldx > K.  fp16: the reference runs on the
    rounded weights, so the fp32 bound holds"""
    E = _E()
    Kd, ROWS, M, norm = E.AR_GEMV_INSTS[inst]
    rng = np.random.default_rng(600 + inst)
    W = (rng.standard_normal((3 * ROWS, Kd)) / np.sqrt(Kd)).astype(F32)
    W[1] = 0.0
    W[1, -4:] = [1.0, -2.0, 3.0, 0.5]
    x = rng.standard_normal((M, Kd)).astype(F32)
    if M == 2:
        x[0] *= 1e4
        x[1] *= 1e-4
    X = np.full((M, Kd + 4), 1e30, F32)
    X[:, :Kd] = x
    nw = rng.uniform(0.5, 1.5, Kd).astype(F32) if norm else None
    out, same = E.test_ar_gemv(inst, W, X, nw, half=half, ldo=3 * ROWS + 3, fill=SENT)
    name = "ardev::gemv<%s>" % ("half" if half else "float")
    shape = "K=%d ROWS=%d M=%d%s" % (Kd, ROWS, M, " norm" if norm else "")
    _exact(name, shape, bool(same.all()), "all 64 lanes hold the same values")
    _exact(name, shape, bool((out[:, 3 * ROWS:] == SENT).all()), "pad untouched")
    kw = dict(norm_w=nw, eps=1e-5, half=half)
    want = R.gemv_ref(x, W, **kw)
    assert np.abs(want[:, 1]).min() > 0                          # the tail-only row contributes
    _check(record_property, name, shape, out[:, :3 * ROWS], want, R.gemv_ref(x, W, dt=F32, **kw))


@pytest.mark.parametrize("half", [False, True])
def test_ardev_gemv_row_offset_beyond_2_31_bytes(half, record_property):
    """WFrag::load at row 700 000: row * K = 5.4e8 elements, past 2^31 / 4 -- a 32-bit element or byte offset would wrap.  The device array is
    allocated whole (2.1 GB of float, 1.1 GB of fp16) and only the rows read are uploaded, so the case costs a malloc"""
    E = _E()
    inst = 6                                                      # (768, 2, 1, -)
    rng = np.random.default_rng(611)
    W = (rng.standard_normal((4, 768)) / np.sqrt(768)).astype(F32)
    x = rng.standard_normal((1, 768)).astype(F32)
    out, same = E.test_ar_gemv(inst, W, x, None, half=half, row0=700000)
    name = "ardev::gemv<%s>" % ("half" if half else "float")
    _exact(name, "row0=700000", bool(same.all()), "all 64 lanes hold the same values")
    _check(record_property, name, "K=768 ROWS=2 M=1 row0=700000", out, R.gemv_ref(x, W, half=half), R.gemv_ref(x, W, half=half, dt=F32))


# =====================================================================================================================================
# token and history kernels
# =====================================================================================================================================
def test_gather_rows_strided_index():
    E = _E()
    rng = np.random.default_rng(51)
    D, rows, ldo = 768, 4, 773
    table = rng.standard_normal((40, D)).astype(F32)
    idx = np.full(rows * 8, 10 ** 6, np.int32)                   # only every 8th entry is read
    picks = np.array([0, 33, 7, 36], np.int32)
    idx[::8] = picks
    out = np.full(rows * ldo, SENT, F32)
    E.test_gather_rows(table, idx, 8, 3, rows, out, ldo)
    o = out.reshape(rows, ldo)
    _exact("launch_gather_rows", "D=768 idx_stride=8 idx_offset=3 ldo=773", bool(np.array_equal(_bits(o[:, :D]), _bits(table[picks + 3]))), "rows == table[idx + offset]")
    _exact("launch_gather_rows", "D=768 idx_stride=8 idx_offset=3 ldo=773", bool((o[:, D:] == SENT).all()), "pad untouched")


@pytest.mark.parametrize("ncb", [1, 8])
@pytest.mark.parametrize("D", [768, 300])
def test_audio_embed_both_stride_forms(D, ncb):
    """launch_audio_embed as the frame's end calls it (codes [rows][ncb]: strides (ncb, 1)) and as the prompt tail does (codes [ncb][Pmax]: strides
    (1, Pmax)); D = 300 leaves the last block of grid.y ragged.  The kernel adds in codebook order: float32 restated on the CPU is bit-exact"""
    E = _E()
    rng = np.random.default_rng(52 + D + ncb)
    cbs, rows, ldo, Pmax = 50, 5, D + 7, 11
    table = rng.standard_normal((ncb * cbs, D)).astype(F32)
    codes = rng.integers(0, cbs, (rows, ncb)).astype(np.int32)
    want = R.audio_embed(table, codes, cbs)
    for form, flat, cs, bs in (("(ncb,1)", codes.reshape(-1), ncb, 1), ("(1,Pmax)", None, 1, Pmax)):
        if flat is None:
            flat = np.full(ncb * Pmax, 10 ** 6, np.int32)
            flat.reshape(ncb, Pmax)[:, 3:3 + rows] = codes.T
            flat = flat[3:]                                       # the launch starts at frame 3 of the stored prompt
        out = np.full(rows * ldo, SENT, F32)
        E.test_audio_embed(table, flat, cs, bs, rows, ncb, cbs, out, ldo)
        o = out.reshape(rows, ldo)
        shape = "D=%d ncb=%d strides %s" % (D, ncb, form)
        _exact("launch_audio_embed", shape, bool(np.array_equal(_bits(o[:, :D]), _bits(want))), "rows == float32 sum in codebook order")
        _exact("launch_audio_embed", shape, bool((o[:, D:] == SENT).all()), "pad untouched")


def _shift_case(rng, descs, B, slices, counter=None, counter_add=0):
    """descs = [(H, T, C, batch pad)] laid out one after another with gaps; -> (ok rows moved, ok rest untouched, counter)"""
    layout, at = [], 5
    for H, T, C, bpad in descs:
        bstride = (H + T) * C + bpad
        layout.append((at, bstride, H, T, C))
        at += B * bstride + 9
    buf = rng.standard_normal(at).astype(F32)
    want = buf.copy()
    for off, bs, H, T, C in layout:
        for b in range(B):
            v = want[off + b * bs: off + b * bs + (H + T) * C].reshape(H + T, C)
            v[:] = R.shift_history(buf[off + b * bs: off + b * bs + (H + T) * C].reshape(H + T, C), H, T)
    got = buf.copy()
    cnt = _E().test_shift_history(got, layout, B, slices, counter, counter_add)
    return bool(np.array_equal(_bits(got), _bits(want))), bool(not np.array_equal(_bits(want), _bits(buf))), cnt


SHIFT_CASES = [("T<H overlap", [(9, 2, 16, 3)], 1), ("T=H", [(6, 6, 16, 3)], 1), ("T>H", [(3, 8, 16, 0)], 1),
               ("H*cs=4095", [(4095, 3, 1, 5)], 1), ("H*cs=4096", [(4096, 3, 1, 5)], 1), ("H*cs=4097", [(4097, 3, 1, 5)], 1), ("H*cs=3*4096+5", [(12293, 7, 1, 0)], 1),
               ("C=512 1 slice", [(9, 2, 512, 12)], 1), ("C=512 4 slices", [(9, 2, 512, 12)], 4), ("C=512 16 slices", [(88, 1, 512, 12)], 16),
               ("C=100 4 slices (no split)", [(50, 3, 100, 4)], 4), ("two descriptors", [(9, 2, 16, 3), (4100, 1, 4, 0)], 1),
               ("two descriptors 4 slices", [(40, 4, 512, 0), (7, 9, 100, 8)], 4)]


@pytest.mark.parametrize("tag,descs,slices", SHIFT_CASES, ids=[c[0] for c in SHIFT_CASES])
def test_shift_history(tag, descs, slices):
    """rows [T, T + H) -> [0, H) in place, B = 3 items at a padded stride: overlapping ranges, the 4096-element pass boundary, column slices;
    rows at and beyond H, the batch pads and the gaps between tensors keep their bits"""
    ok, moved, _ = _shift_case(np.random.default_rng(len(tag)), descs, 3, slices)
    assert moved
    _exact("launch_shift_history", tag, ok, "rows [0, H) == rows [T, T + H) of the input; everything else untouched")


def test_shift_history_counter_forms():
    rng = np.random.default_rng(53)
    ok, _, cnt = _shift_case(rng, [(9, 2, 16, 3)], 3, 1, counter=41, counter_add=1)
    _exact("launch_shift_history", "counter += 1", ok and cnt == 42, "tensor shifted and the counter bumped once")
    ok, moved, cnt = _shift_case(rng, [], 3, 1, counter=41, counter_add=1)
    _exact("launch_shift_history", "n_desc=0 counter += 1", ok and not moved and cnt == 42, "no tensor: only the counter bumped")
    ok, moved, cnt = _shift_case(rng, [], 3, 1)
    _exact("launch_shift_history", "n_desc=0 no counter", ok and not moved and cnt is None, "nothing to do")


@pytest.mark.parametrize("n", [3, 300])
def test_ring_write_every_origin(n):
    """a ring of 5 chunks (n = 3 samples; n = 300: two workgroups per item): every origin, a null step (origin 0), and a muted slot whose chunk --
    a NaN block here -- is not read: it gets zeros"""
    E = _E()
    rng = np.random.default_rng(54 + n)
    B, N = 3, 5 * n
    for step in (None, 0, 1, 2, 3, 4, 5, 6, 1000003):
        ring0 = rng.standard_normal((B, N)).astype(F32)
        chunk = rng.standard_normal((B, n)).astype(F32)
        ring = ring0.copy()
        E.test_ring_write(ring, chunk, step)
        _exact("launch_ring_write", "n=%d step=%s" % (n, step), bool(np.array_equal(_bits(ring), _bits(R.ring_write(ring0, chunk, step or 0)))), "ring == reference")
    ring0 = rng.standard_normal((B, N)).astype(F32)
    chunk = rng.standard_normal((B, n)).astype(F32)
    want = chunk.copy()
    want[1] = 0.0
    chunk[1] = np.nan
    ring = ring0.copy()
    E.test_ring_write(ring, chunk, 7, slot_flag=[0, 1, 2])        # slot 1 input-muted; slot 2 carries the OUTPUT flag only: written normally
    _exact("launch_ring_write", "n=%d muted slot" % n, bool(np.array_equal(_bits(ring), _bits(R.ring_write(ring0, want, 7)))), "muted slot gets zeros, its chunk is not read")


@pytest.mark.parametrize("T", [10, 300])
def test_conv_post_tanh_output_muted_slot(T):
    """kSlotOutputMuted on one of three slots: its PCM rows are zeros, the other slots and everything outside the rows keep the bits of the unflagged run"""
    E = _E()
    B, C, k = 3, 32, 7
    rng = np.random.default_rng(55 + T)
    x = (rng.standard_normal((B, T + k - 1, C)) * 2).astype(F32)
    w = (rng.standard_normal((k, C)) * 0.12).astype(F32)
    bias = np.array([0.03], F32)
    xb, pb, p_off = (T + k - 1) * C, T + 11, 5
    runs = []
    for flag in (None, [0, 2, 1], [0, 0, 0]):
        pcm = np.full((B - 1) * pb + p_off + T + 4, SENT, F32)
        E.test_conv_post(x.reshape(-1), pcm, B, T, C, k, w, bias, xb, 0, pb, p_off, slot_flag=flag)
        runs.append(pcm)
    plain, muted, zeros = runs
    want = plain.copy()
    want[pb + p_off: pb + p_off + T] = 0.0
    assert np.abs(plain[pb + p_off: pb + p_off + T]).min() > 0
    _exact("conv_post_tanh", "T=%d slot_flag" % T, bool(np.array_equal(_bits(muted), _bits(want))), "muted slot zeros, the rest as without flags")
    _exact("conv_post_tanh", "T=%d slot_flag all zero" % T, bool(np.array_equal(_bits(zeros), _bits(plain))), "zero flags change nothing")
