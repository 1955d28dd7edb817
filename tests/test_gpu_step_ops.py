"""The glue of the chunk step, kernel by kernel: the 22 bookkeeping kernels of csrc/engine_kernels.hip through their launchers (hook
sva_test_step_ops: the grid and block size the engine uses) and the fused HiFiGAN level voc_level_kernel<16 | 32> through launch_voc_level (hook
sva_test_voc_level), against the references of tests/kernel_refs.py, which tests/test_kernel_refs.py pins to the oracle on the CPU.

The bookkeeping kernels copy, count and add float32 embeddings in codebook order: every array a kernel may write is compared WHOLE and EXACTLY
(bit patterns for floats), so a write outside the expected entries shows as a changed sentinel.  The cases and their preconditions live in
tests/step_ops_cases.py.  The level's branch outputs are compared with float64 under the one derived bound of test_gpu_kernels.py,
4 e32 + 4 ulp32(max |ref|), e32 from the same chain evaluated naively in float32 on the CPU.  Every refusal is a host-side check: nothing is launched.

With SVA_STEP_OPS_PARITY_TABLE=<path> the run writes its table there (profiles/step_ops_parity.txt)."""
import os
import time

import numpy as np
import pytest

import kernel_refs as R
import step_ops_cases as S
import test_gpu_kernels as K

pytestmark = pytest.mark.gpu

F32, F64, I32 = np.float32, np.float64, np.int32
_TABLE = []          # (kernel, shape, exact property or "", err, bound, ratio)


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    t0 = time.time()
    yield
    path = os.environ.get("SVA_STEP_OPS_PARITY_TABLE")
    if path and _TABLE:
        floats = [t for t in _TABLE if not t[2]]
        with open(path, "w") as f:
            f.write("# %d cases (%d compared with float64, %d exact checks), worst err / bound = %.3f, wall %.1f s\n" %
                    (len(_TABLE), len(floats), len(_TABLE) - len(floats), max(t[5] for t in _TABLE), time.time() - t0))
            f.write("%-26s %-72s %12s %12s %8s\n" % ("kernel", "shape", "max_err", "bound", "ratio"))
            worst = {}
            for k, s, what, e, b, r in floats:          # the worst case per kernel
                if k not in worst or r > worst[k][3]:
                    worst[k] = (s, e, b, r)
            for k, (s, e, b, r) in worst.items():
                f.write("%-26s %-72s %12.4e %12.4e %8.3f\n" % (k, s, e, b, r))
            f.write("\n%-26s %-92s %6s %6s\n" % ("kernel", "exact property", "held", "failed"))
            rows = {}
            for k, s, what, e, b, r in _TABLE:
                if what:
                    c = rows.setdefault((k, what), [0, 0])
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


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# =====================================================================================================================================
# the bookkeeping kernels
# =====================================================================================================================================
_CASES = S.all_cases()          # built once; every run works on copies


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_step_op_is_exact(case):
    """one launch through the kernel's launcher: every array it may write comes back equal to the reference's, whole -- the written entries, and
    the sentinels of everything else (untouched slots, ring entries outside the written ones, rows behind the last, padding of the strides)"""
    arrays = [None if a is None else a.copy() for a in case["arrays"]]
    _E().test_step_op(case["op"], case["desc"], arrays)
    for i in case["io"]:
        ok = _same_bits(arrays[i], case["want"][i])
        if not ok:
            bad = np.flatnonzero(arrays[i].reshape(-1) != case["want"][i].reshape(-1))
            print(case["id"], "array", i, "first differing entries", bad[:8], arrays[i].reshape(-1)[bad[:8]], case["want"][i].reshape(-1)[bad[:8]])
        _exact(case["op"], case["id"].split(" ", 1)[1], ok, "%s whole and exact (written entries and every sentinel around them)" % S.ARRAYS[case["op"]][i])
    for i, a in enumerate(case["arrays"]):
        if a is not None and i not in case["io"]:
            assert _same_bits(arrays[i], a)          # (inputs are not downloaded: the hook left the host copies alone)


def _first(op, pred=lambda c: True):
    c = next(c for c in _CASES if c["op"] == op and pred(c))
    return c, [None if a is None else a.copy() for a in c["arrays"]]


def _refused(op, desc, arrays):
    E = _E()
    before = [None if a is None else a.copy() for a in arrays]
    with pytest.raises(E.Refused):
        E.test_step_op(op, desc, arrays)
    ok = all(a is None or _same_bits(a, b) for a, b in zip(arrays, before))
    _exact(op, "refusal", ok, "refused on the host, nothing written")


def test_step_op_refusals():
    """what a launch would index with is checked on the host: a code outside its table, a slot outside the batch, a capacity that is no power of two,
    more than 128 slots in a pass, more than 8 codebooks, a row offset table that is not the running sum (na < 0 cannot be laid out), na < d"""
    c, a = _first("ar_prepare_step")
    a[2][0, c["desc"][2]] = S.NC          # codes[0][code_off] one past the content table
    _refused(c["op"], c["desc"], a)
    c, a = _first("build_prompt")
    a[4][1] = S.NC
    _refused(c["op"], c["desc"], a)
    c, a = _first("build_prompt")
    a[5][0, 0] = S.CBS          # an audio code one past its codebook
    _refused(c["op"], c["desc"], a)
    c, a = _first("build_delayfill", lambda c: c["desc"][0] > 1)
    a[5][0] = c["desc"][0]          # a listed slot == B
    _refused(c["op"], c["desc"], a)
    c, a = _first("build_delayfill")
    a[1][0, 3] = -1          # a ring entry that is no content code
    _refused(c["op"], c["desc"], a)
    for op, i_cap in (("ar_finish_frame", 2), ("append_content", 3), ("put_codes", 3), ("build_delayfill", 4), ("build_reprefill", 7), ("finish_reprefill", 7)):
        c, a = _first(op, lambda c: c["desc"][i_cap] == 16)
        d = list(c["desc"])
        d[i_cap] = 12          # not a power of two (the arrays are large enough for it: 12 < 16)
        _refused(op, d, a)
    for op in ("build_reprefill", "finish_reprefill"):
        c, a = _first(op, lambda c: c["desc"][1] == 3)
        a[0][1] = c["desc"][0]          # slot == B
        _refused(op, c["desc"], a)
        c, a = _first(op, lambda c: c["desc"][1] == 3)
        a[3][2] = c["desc"][2] - 1          # na < d
        _refused(op, c["desc"], a)
        c, a = _first(op, lambda c: c["desc"][1] == 3)
        a[3][0] = -1          # a negative na: the row offsets would not be monotone
        _refused(op, c["desc"], a)
        c, a = _first(op, lambda c: c["desc"][1] == 128)
        d = list(c["desc"])
        d[1] = 129          # (the per-slot arrays hold 128 entries: the hook refuses on the count alone)
        _refused(op, d, a)
        c, a = _first(op, lambda c: c["desc"][3] == 8)
        d = list(c["desc"])
        d[3] = 9          # ncb > 8
        _refused(op, d, a)
    c, a = _first("add_list")
    a[1][0] = c["desc"][0]
    _refused(c["op"], c["desc"], a)
    c, a = _first("set_slot_i32")
    d = list(c["desc"])
    d[2] = d[0]
    _refused(c["op"], d, a)
    c, a = _first("put_row")
    d = list(c["desc"])
    d[1] = d[0]
    _refused(c["op"], d, a)
    c, a = _first("copy_tokens")
    d = list(c["desc"])
    d[2] += 1          # a gap that pushes the newest tokens past the end of tok
    _refused(c["op"], d, a)
    c, a = _first("mean3", lambda c: c["desc"][4] > 0)
    d = list(c["desc"])
    d[4] += 12          # o_off that pushes the last lanes past the end of out
    _refused(c["op"], d, a)


@pytest.mark.parametrize("op", ["build_reprefill", "finish_reprefill"])
def test_reprefill_refuses_a_stored_prompt_shorter_than_the_delay(op):
    """Rt < d: the audio rows of frames Rt .. d - 1 of the new prompt are wait4start rows (DualAR.prefill_prompt; pinned on the CPU by
    test_row_builder_refs_are_the_oracles_sequences), which the one-pass row builder does not hold, and the prompt upload leaves the ref_tail entries
    in front of frame 0 unset.  The launchers refuse it -- SlotBook::one_pass_ok sends such a slot through the whole-prompt prefill, which builds
    those rows (build_prompt) -- so ref_tail is never read where it was not written."""
    c, a = _first(op, lambda c: c["desc"][1] == 3 and c["desc"][2] >= 2)
    a[1][1] = c["desc"][2] - 1
    _refused(op, c["desc"], a)


# =====================================================================================================================================
# the fused HiFiGAN level
# =====================================================================================================================================
_VOC = S.voc_cases()
_WEIGHTS = {C: S.voc_weights(C) for C in (16, 32)}


def _flat_weights(C):
    W, bias = _WEIGHTS[C]
    return np.concatenate([w.reshape(-1) for br in W for w in br]), np.stack([b for br in bias for b in br])


def _launch_level(c, x, W=None, xH=S.RF_MAX, rows_per_frame=None):
    """x [B, rows, C] (rows = x_bstride / C) -> (the three outputs [3, B, y rows, C] with their sentinels, the tile height)"""
    E = _E()
    C, B, Tl = c["C"], c["B"], c["Tl"]
    Wf, bf = _flat_weights(C) if W is None else W
    y_rows = Tl + 2          # y_bstride: two padding rows per stream
    Y3 = [np.full(B * y_rows * C, S.SENT, F32) for _ in range(3)]
    TR = E.test_voc_level(np.ascontiguousarray(x.reshape(-1)), Y3, Wf, bf, C, B, Tl, xH, x.shape[1] * C, y_rows * C, S.DIL,
                          c["rows_per_frame"] if rows_per_frame is None else rows_per_frame, c["frames_done"])
    return np.stack([y.reshape(B, y_rows, C) for y in Y3]), TR


@pytest.mark.parametrize("c", _VOC, ids=["C %(C)d B %(B)d Tl %(Tl)d frames_done %(frames_done)d rows_per_frame %(rows_per_frame)d %(kind)s" % c for c in _VOC])
def test_voc_level_vs_float64(c, record_property):
    """one launch = six chained convs per branch in LDS: the branch outputs against the float64 chain, the rows of Y3 behind Tl and the other
    streams' padding bit-identical, the tile height the launcher's rule gives.  frames_done = 0: the history rows hold NaN, which any read of
    them would carry into the output"""
    C, B, Tl = c["C"], c["B"], c["Tl"]
    tag = "C %d B %d Tl %d fd %d rpf %d %s" % (C, B, Tl, c["frames_done"], c["rows_per_frame"], c["kind"])
    x = S.voc_input(c)
    got, TR = _launch_level(c, x)
    _exact("voc_level", tag, TR == S.voc_tile_rows(C, B, Tl) and TR == (128 if c["kind"] == "next tile height" else 64), "tile height follows the launcher's rule")
    _exact("voc_level", tag, bool((got[:, :, Tl:] == S.SENT).all()), "rows of Y3 behind Tl untouched")
    W, bias = _WEIGHTS[C]
    xin = x[:, :S.RF_MAX + Tl]
    before = c["frames_done"] * c["rows_per_frame"]
    f64 = R.voc_level(xin, W, bias, S.DIL, before)
    f32 = R.voc_level(xin, W, bias, S.DIL, before, dt=F32)
    assert np.isfinite(f64).all()
    if c["kind"] == "zero":          # a zero input is the bias chain: still compared, and the same in every row behind the halo
        assert np.abs(f64).max() > 0
    for br in range(3):
        _check(record_property, "voc_level k=%d" % R.VOC_LEVEL_K[br], tag, got[br, :, :Tl], f64[br], f32[br])


def test_voc_level_zero_forcing_at_the_stream_start(record_property):
    """frames_done = 0: every row in front of the stream start is zero in all six intermediates, whatever the history holds.  The same launch with
    the history rows zero, NaN and huge must give bit-identical outputs, equal to the float64 chain over a zero-padded stream; with frames_done = 1 the
    same (finite) history rows are inside the stream and must change the first rows"""
    for C in (16, 32):
        c = dict(C=C, B=1, Tl=40, frames_done=0, rows_per_frame=180, kind="normal")
        x = S.voc_input(c)
        outs = []
        for fill in (np.nan, 0.0, 1e30):
            x[:, :S.RF_MAX] = fill
            outs.append(_launch_level(c, x)[0])
        _exact("voc_level", "C %d stream start" % C, _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2]), "history rows in front of the stream start never read")
        x[:, :S.RF_MAX] = np.random.default_rng(C).standard_normal((1, S.RF_MAX, C)).astype(F32)
        c1 = dict(c, frames_done=1)
        got1 = _launch_level(c1, x)[0]
        W, bias = _WEIGHTS[C]
        f64 = R.voc_level(x[:, :S.RF_MAX + 40], W, bias, S.DIL, 180)
        f32 = R.voc_level(x[:, :S.RF_MAX + 40], W, bias, S.DIL, 180, dt=F32)
        for br in range(3):
            _check(record_property, "voc_level k=%d" % R.VOC_LEVEL_K[br], "C %d history inside the stream" % C, got1[br, :, :40], f64[br], f32[br])
        assert np.abs(got1[:, :, :40] - outs[0][:, :, :40]).max() > 1e-3


@pytest.mark.parametrize("what", ["C", "xH", "rows_per_frame"])
def test_voc_level_refusals(what):
    E = _E()
    c = dict(C=16, B=1, Tl=16, frames_done=1, rows_per_frame=180, kind="normal")
    x = S.voc_input(c)
    with pytest.raises(E.Refused):
        if what == "C":
            c48 = dict(c, C=48)
            rng = np.random.default_rng(0)
            Wf = (rng.standard_normal(6 * 21 * 48 * 48) * 0.01).astype(F32)
            _launch_level(c48, np.zeros((1, S.RF_MAX + 16 + 3, 48), F32), W=(Wf, np.zeros((18, 48), F32)))
        elif what == "xH":
            _launch_level(c, x[:, 1:], xH=S.RF_MAX - 1)
        else:
            _launch_level(c, x, rows_per_frame=S.RF_MAX - 1)
    _exact("voc_level", "refusal: " + what, True, "refused on the host")
