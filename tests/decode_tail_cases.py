"""Inputs of the sampler tests of test_gpu_decode_tail.py, shared with the CPU test that asserts every one of their rows DECIDABLE
(kernel_refs.nucleus_token; test_kernel_refs.py): the GPU tests compare tokens exactly, so no row may sit where float32 rounding inside a
kernel could legitimately pick another token.  Seeds were chosen on the CPU until that holds; the CPU test keeps it true."""
import numpy as np

import kernel_refs as R

F32 = np.float32
RANDOM_SETTINGS = ((0.7, 0.7), (0.9, 1.0), (0.05, 0.7), (1.0, 0.7), (0.999, 1.3))          # (top_p, temperature)
HARD_SETTINGS = ((0.7, 0.7), (0.3, 1.3), (1.0, 0.7), (0.999, 0.5), (0.05, 0.7))
V_SMALL = (1, 63, 1000, 1024)           # nucleus_sample<4,4>, <1,16>, launch_sampler_small
V_LARGE = (4097, 8191, 8192)            # nucleus_sample<4,32>, <8,16>, launch_sampler (threshold search)
V_SORT = (2048, 8193)                   # launch_sampler alone: the LDS sort with its dynamic LDS
V_ALL = V_SMALL + V_LARGE + V_SORT
RANDOM_ROWS = 16                        # rows of random_rows the GPU tests run (the CPU test covers all 48)


def random_rows(V, rows=48):
    """the generator of test_sampler_implementations_vs_oracle_and_each_other"""
    rng = np.random.default_rng(V)
    L = (rng.standard_normal((rows, V)) * rng.uniform(0.5, 8.0, (rows, 1))).astype(F32)
    Q = (rng.exponential(1.0, (rows, V)) + 1e-9).astype(F32)
    return L, Q


HARD_NAMES = ("uniform", "rounded", "tie at the top", "all but four underflow", "half-integer classes", "two huge classes", "-inf at 10 %",
              "one-token nucleus", "keep-all (mass == 1.0f)", "cut in a tie class over the ragged slot")
HARD_SEEDS = {1: 0, 63: 1122, 1000: 93, 1024: 18, 4097: 0, 8191: 33, 8192: 0, 2048: 7, 8193: 4}       # the first seed at which every row is decidable


def hard_rows(V, seed=None):
    """[10, V] logits and noise: the six rows of the existing sampler test, then a row with -inf at a tenth of the ids, a peaked row whose
    nucleus is one token, a row of 2^k equal logits among -inf (float32 probabilities 2^-k exactly: their sum is 1.0f, which does not exceed
    top_p = 1.0 -- the keep-all branch) and a row (one token at p = 1/2, eight tied at 1/16 on the last ids, V - 8 .. V - 1) whose cut falls
    inside the tie class that occupies the last, ragged slot of every kernel's element layout"""
    rng = np.random.default_rng(HARD_SEEDS[V] if seed is None else seed)
    T = (rng.standard_normal((10, V)) * rng.uniform(0.5, 8.0, (10, 1))).astype(F32)
    Q = (rng.exponential(1.0, (10, V)) + 1e-9).astype(F32)
    ix = lambda i: min(i, V - 1)
    T[0, :] = 0.25
    T[1, :] = np.round(T[1, :])
    T[2, ix(17)] = T[2, ix(911)] = T[2, ix(5)] = T[2].max() + 3.0
    T[3, :] = -200.0
    T[3, ix(40):ix(40) + 4] = 0.0
    T[4, :] = np.floor(T[4, :] * 2) / 2
    T[5, :] = 1e4 * np.sign(T[5, :])
    if V >= 10:
        T[6, rng.choice(V, V // 10, replace=False)] = -np.inf
    T[7, :] = (T[7, :] / max(float(np.abs(T[7]).max()), 1.0)).astype(F32)
    T[7, V // 3] = 12.0
    k = 1
    while 4 * k <= V:
        k *= 2
    T[8, :] = -np.inf
    T[8, 0:2 * k:2][:k] = 0.0                           # k = 2^j equal logits on even ids (V = 1: the one id)
    if V >= 16:
        T[9, :] = -np.inf
        T[9, 3] = np.log(8.0)
        T[9, V - 8:] = 0.0
    return T, Q


# ---- device RNG: rows whose noise is the counter generator's (synth_weights.exp1_noise) ----
RNG_SEEDS = {1000: 0, 8192: 0, 2048: 0}


def rng_case(V, kind, cb, base=None):
    """4 rows, per-row distinct (seed, frame); noise_elem_off = cb V -> (L, Q = the host twin's draws, seed uint64 [4], frame int32 [4], off)"""
    from streamvoiceanon_amd.synth_weights import exp1_noise
    base = RNG_SEEDS[V] if base is None else base
    rng = np.random.default_rng(7000 + 13 * base + V)
    L = (rng.standard_normal((4, V)) * rng.uniform(0.5, 8.0, (4, 1))).astype(F32)
    seed = np.array([1000 + 37 * base + 7 * r for r in range(4)], np.uint64)
    frame = np.array([3 + 5 * r + base for r in range(4)], np.int32)
    off = cb * V
    Q = np.stack([exp1_noise(int(seed[r]), int(frame[r]), kind, off + V)[off:] for r in range(4)])
    return L, Q, seed, frame, off


# ---- the production form of the codebook head: [B = 3][8][1000] logits, codebook 5 ----
PROD_SEED = 0
PROD = dict(B=3, ncb=8, cbs=1000, cb=5, vocab=8192, chunk=2, D=768)


def production_case(seed=None):
    """-> (logits [B, ncb, cbs], noise [B, vocab + ncb cbs] as a step's noise row)"""
    p = PROD
    rng = np.random.default_rng(9100 + (PROD_SEED if seed is None else seed))
    L = (rng.standard_normal((p["B"], p["ncb"], p["cbs"])) * rng.uniform(0.5, 8.0, (p["B"], p["ncb"], 1))).astype(F32)
    Q = (rng.exponential(1.0, (p["B"], p["vocab"] + p["ncb"] * p["cbs"])) + 1e-9).astype(F32)
    return L, Q


def production_rows(seed=None):
    p = PROD
    L, Q = production_case(seed)
    o = p["vocab"] + p["cb"] * p["cbs"]
    return L[:, p["cb"], :], Q[:, o:o + p["cbs"]]


# ---- logit edits in front of the sampler ----
EDIT_SEEDS = {1000: 0, 8192: 0}
EDIT_PENALTY = 1.5


def edits_case(V, seed=None):
    """3 rows; prev with duplicates, -1 entries and one id >= V; a suppress list for the token head (V = 8192) only, as stages.hip runs it
    -> (L, Q, prev, suppress)"""
    rng = np.random.default_rng(9300 + V + 17 * (EDIT_SEEDS[V] if seed is None else seed))
    L = (rng.standard_normal((3, V)) * rng.uniform(0.5, 4.0, (3, 1))).astype(F32)
    Q = (rng.exponential(1.0, (3, V)) + 1e-9).astype(F32)
    top = np.argsort(-L, axis=1)[:, :6].reshape(-1)                  # penalise what would otherwise win
    prev = np.concatenate([top, top[:5], [-1, V + 3, -1], rng.integers(0, V, 40)]).astype(np.int32)
    sup = np.concatenate([np.argsort(-L[0])[6:9], [-2, V, V + 100]]).astype(np.int32) if V > 1024 else np.zeros(0, np.int32)
    return L, Q, prev, sup


def edited_rows(V, seed=None):
    L, Q, prev, sup = edits_case(V, seed)
    return np.stack([R.logit_edits(L[r], prev, sup, EDIT_PENALTY) for r in range(L.shape[0])]), Q


def all_sampler_cases():
    """every (tag, logits [rows, V], noise [rows, V], top_p, temperature) a GPU sampler test compares exactly"""
    for V in V_ALL:
        L, Q = random_rows(V)
        for tp, temp in RANDOM_SETTINGS:
            yield "random V=%d" % V, L, Q, tp, temp
        T, Qh = hard_rows(V)
        for tp, temp in HARD_SETTINGS:
            yield "hard V=%d" % V, T, Qh, tp, temp
    for V in sorted(RNG_SEEDS):
        for kind in (0, 1):
            for cb in (0, 7):
                L, Q, _, _, _ = rng_case(V, kind, cb)
                yield "rng V=%d kind=%d cb=%d" % (V, kind, cb), L, Q, 0.7, 0.7
    L, Q = production_rows()
    yield "production", L, Q, 0.7, 0.7
    for V in sorted(EDIT_SEEDS):
        L, Q = edited_rows(V)
        yield "edits V=%d" % V, L, Q, 0.7, 0.7


def undecidable(L, Q, tp, temp):
    """rows of (L, Q) that are not decidable, with their lead"""
    bad = []
    for r in range(L.shape[0]):
        _, ok, lead = R.nucleus_token(L[r], Q[r], temp, tp)
        if not ok:
            bad.append((r, lead))
    return bad
