"""voc_conv_kernel (csrc/gemm_planes.hip: one ResBlock conv stage of a narrow HiFiGAN level, C = 16 / 32, over row-major operand planes) alone against
float64, through launch_voc_conv itself (sva_test_voc_conv -> engine.test_voc_conv): its four instantiations {H3, H1} x {C = 32 / 128-row tiles,
C = 16 / 256-row tiles}, and the row-major arm of to_planes_act_kernel (blocked = 0) that makes its input.  Cases and the comparison rule live in
tests/voc_conv_cases.py; tests/test_kernel_refs.py pins the reference to torch's conv1d and shows on the CPU that the rule catches a reversed tap
order, a dilation or a first row off by one, a residual from the wrong stream and a last odd tap counted twice.

Rule (_pl_verify of test_gpu_conv_gemm.py, unchanged): the reference is float64 on the operands AS THE PLANES HOLD THEM (the returned Ap decoded,
kernel_refs.weight_planes -- which the returned weight planes must decode to, with exact zeros in the C = 16 pad columns); every floating comparison
goes through _check: err <= 4 e32 + 4 ulp32 + extra, extra = the dropped lo x lo product (H3) / 0 (H1), capped by 3e-6 (H3) / 2e-3 (H1) of max |ref|.
Exact: everything outside the written rows of Cf / Cp keeps its sentinel, res comes back as it went in, a repeated launch and a launch on another
grid give the same bits, a refusal writes nothing.

With SVA_VOC_CONV_PARITY_TABLE=<path> the run writes its table there (profiles/voc_conv_parity.txt): one row per comparison."""
import os
import time

import numpy as np
import pytest

import kernel_refs as R
import test_gpu_kernels as K
import voc_conv_cases as V

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INST = [(C, name) for C in (32, 16) for name in ("H3", "H1")]
inst = pytest.mark.parametrize("C,mname", INST, ids=["C%d-%s" % i for i in INST])
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    t0 = time.time()
    yield
    path = os.environ.get("SVA_VOC_CONV_PARITY_TABLE")
    if path and _TABLE:
        floats = [r for r in _TABLE if r[3] > 0.0]
        with open(path, "w") as f:
            f.write("# %d rows (%d compared with float64, %d exact checks), wall %.1f s.  Worst err / bound per instantiation:\n" %
                    (len(_TABLE), len(floats), len(_TABLE) - len(floats), time.time() - t0))
            for k in sorted(set(r[0] for r in floats)):
                f.write("#   %-34s %.3f\n" % (k, max(r[4] for r in floats if r[0] == k)))
            f.write("%-34s %-58s %12s %12s %8s\n" % ("kernel", "shape", "max_err", "bound", "ratio"))
            for k, s, e, b, r in _TABLE:
                f.write("%-34s %-58s %12.4e %12.4e %8.3f\n" % (k, s, e, b, r))


def _mine(fn, *a, **kw):
    """the comparison helpers of test_gpu_kernels.py, their table rows moved into this module's table"""
    n = len(K._TABLE)
    try:
        return fn(*a, **kw)
    finally:
        _TABLE.extend(K._TABLE[n:])
        del K._TABLE[n:]


def _check(*a, **kw):
    return _mine(K._check, *a, **kw)


def _exact(*a, **kw):
    return _mine(K._exact, *a, **kw)


def _name(C, mname):
    return "voc_conv %s C=%d" % (mname, C)


def _operands(h, mode, exact_split=True):
    """(a, |a lo|, w, |w lo|) from the planes the hook returned.  The weight planes must be make_weight_planes' (restated by kernel_refs.weight_planes),
    K-blocked, the C = 16 pad columns exactly zero; with exact_split the input planes must be the CPU split of A"""
    npl, C, taps = V.n_planes(mode), h["C"], h["taps"]
    rows_n, K_, Kp = h["B"] * h["a_rows_b"], taps * C, V.padded_k(C, taps)
    P = h["Ap"].reshape(npl, -1)
    if exact_split:
        assert np.array_equal(P, V.split_bits(h["A"], npl).reshape(npl, -1)), "A planes differ from the CPU split"
    hi = R.planes_decode(P[:1], 1, rows_n, C, False)
    lo = R.planes_decode(P[1:], 1, rows_n, C, False) if npl == 2 else np.zeros_like(hi)
    whi, wlo = R.weight_planes(h["W"], npl)
    inv = 2.0 ** -V.weight_exp(h["W"])
    Wd = h["Wp"].reshape(npl, -1)
    for p, want in enumerate((whi, wlo)[:npl]):
        got = R.planes_decode(Wd[p:p + 1], 1, C, Kp, True)
        assert np.array_equal(got[:, :K_] * inv, want), "weight planes differ from make_weight_planes"
        assert (got[:, K_:] == 0).all() and not np.signbit(got[:, K_:]).any(), "pad columns of the weight planes are not zero"
    assert Kp == K_ or (C == 16 and taps % 2 == 1 and Kp == K_ + 16)
    return hi + lo, np.abs(lo), whi + wlo, np.abs(wlo)


def _verify(record_property, h, mode, name, tag, exact_split=True):
    """one member's outputs: Cf and the SiLU'd planes under the rule, everything else untouched"""
    a, alo, w, wlo = _operands(h, mode, exact_split)
    q = V.rule(h, mode, a, alo, w, wlo)
    if "Cf" in h:
        idx = V.cf_index(h)
        _check(record_property, name, tag + " Cf", h["Cf"][idx], q["v64"], q["v32"], extra=q["extra"], ceiling=q["ceiling"])
        mask = np.ones(h["Cf"].size, bool)
        mask[idx.reshape(-1)] = False
        _exact(name, tag, bool((h["Cf"][mask] == V.SENT).all()), "Cf outside the written rows unchanged")
    if "Cp" in h:
        npl, C = V.n_planes(mode), h["C"]
        rows_n = h["B"] * h["c_rows_b"]
        planes = h["Cp"].reshape(npl, rows_n, C)
        got = R.planes_decode(planes.reshape(npl, -1), npl, rows_n, C, False)
        rows = V.cp_rows(h)
        _check(record_property, name, tag + " Cp", got[rows], q["s64"], q["s32"], extra=q["extra_p"], ceiling=q["ceiling_p"])
        if "Cp_in" not in h:        # (a case that pre-fills the planes itself compares them itself)
            mask = np.ones(rows_n, bool)
            mask[rows.reshape(-1)] = False
            _exact(name, tag, bool((planes[:, mask] == V.SENT_P).all()), "Cp outside the written rows unchanged")
    if "res" in h:
        _exact(name, tag, np.array_equal(h["res"], h["res_in"]), "res unchanged")


def _run(record_property, ms, mode, name, tag, **kw):
    """one launch (twice) of a group of members made by voc_conv_cases: every member verified"""
    hs = [V.hook(m, mode) for m in ms]
    ovf = np.zeros(1, np.int32)
    r = K._E().test_voc_conv(hs, ms[0]["C"], mode, ms[0]["B"], ms[0]["T"], repeat=True, ovf=ovf, **kw)
    assert not r["refused"], (name, tag, K._last_error())
    for i, h in enumerate(hs):
        _verify(record_property, h, mode, name, "%s #%d k=%d d=%d" % (tag, i, h["taps"], h["dil"]))
    _exact(name, tag, r["identical"] is True, "second launch bit-identical")
    _exact(name, tag, int(ovf[0]) == 0, "overflow word stays 0 on finite outputs")
    return hs


@inst
def test_three_stage_forms_every_dilation(C, mname, record_property):
    """the engine's stages -- c1: bias, SiLU'd planes only; c2: bias + residual, fp32 rows and planes; the last c2: fp32 rows only -- as groups of
    taps (3, 7, 11) handed over in ASCENDING order (the launcher sorts by descending taps: every member's output must still land in its own arrays),
    every branch at every dilation of (1, 3, 5), a different one per member; each form at one and three streams, one and three tiles per stream"""
    mode, tile = V.MODES[mname], V.TILE[C]
    sizes = ((1, tile), (3, tile), (1, 3 * tile))
    for fi, form in enumerate(V.FORMS):
        for rot in range(3):
            dils = V.RES_D[rot:] + V.RES_D[:rot]
            B, T = sizes[(fi + rot) % 3]
            ms = V.group(1000 + 100 * fi + 10 * rot + C, C, B, T, V.RES_K, dils, form)
            _run(record_property, ms, mode, _name(C, mname), "%s B=%d T=%d" % (form, B, T))


@inst
def test_tile_walk_on_one_cu_and_on_the_device(C, mname, record_property):
    """B = 3 streams of three tiles: with cu_limit = 1 (the grid of a CU-masked stream) a branch has one or two workgroups, each walking the tiles
    of its branch through the `tile += nw` loop and the barrier that protects the image; with cu_limit = 0 one workgroup per tile.  Both against
    float64, both twice, and the two grids give the same bits"""
    mode, T = V.MODES[mname], 3 * V.TILE[C]
    ms = V.group(2000 + C, C, 3, T, V.RES_K, (5, 1, 3), "c2")
    name = _name(C, mname)
    one = _run(record_property, ms, mode, name, "walk cu_limit=1 B=3 T=%d" % T, cu_limit=1)
    dev = _run(record_property, ms, mode, name, "walk cu_limit=0 B=3 T=%d" % T, cu_limit=0)
    _exact(name, "walk", all(np.array_equal(a["Cf"], b["Cf"]) and np.array_equal(a["Cp"], b["Cp"]) for a, b in zip(one, dev)), "the two grids bit-identical")


@inst
def test_groups_of_one_two_and_equal_taps(C, mname, record_property):
    mode, tile, name = V.MODES[mname], V.TILE[C], _name(C, mname)
    _run(record_property, V.group(3000 + C, C, 3, tile, (7,), (3,), "c2"), mode, name, "single B=3")
    _run(record_property, V.group(3100 + C, C, 1, 3 * tile, (3, 11), (5, 1), "c2"), mode, name, "pair B=1")
    _run(record_property, V.group(3200 + C, C, 3, tile, (7, 7, 7), (1, 3, 5), "c2"), mode, name, "equal taps B=3")


@inst
def test_tap_and_halo_edges(C, mname, record_property):
    """taps = 1: no halo (C = 16: a single K step whose second tap is clamped onto zero weights); taps = 2: at C = 16 no pad column; taps = 11 at
    dilation 5 and taps = 6 at dilation 10: the 50-row halo, the image fills its LDS rows exactly"""
    mode, tile, name = V.MODES[mname], V.TILE[C], _name(C, mname)
    _run(record_property, V.group(4000 + C, C, 3, tile, (1, 2, 11), (2, 7, 5), "c2"), mode, name, "edges B=3")
    _run(record_property, V.group(4100 + C, C, 1, 3 * tile, (6,), (10,), "c2"), mode, name, "halo 50 = 5 x 10 B=1")
    _run(record_property, V.group(4200 + C, C, 1, tile, (1,), (1,), "c1"), mode, name, "taps=1 alone B=1")


@inst
def test_chained_stages_hand_planes_over(C, mname, record_property):
    """c1 then c2 the way the engine chains them: the input planes are silu(X) -- history rows already there, the T new rows split by to_planes_act
    with SiLU over those rows only --, c1 writes the planes of silu(t) behind t's own history rows, c2 reads them (its reference: the planes c1
    returned, decoded), adds the residual X and writes fp32 rows and planes"""
    mode, T, name = V.MODES[mname], V.TILE[C], _name(C, mname)
    npl, B, taps, dil = V.n_planes(mode), 3, 7, 3
    padL = (taps - 1) * dil
    E = K._E()
    m1 = V.member(5100 + C, C, B, T, taps, dil, idx=1, bias=True, Cp=True, conv=2)
    H = m1["a_row0"] + padL                                   # X: H history rows, then the T new ones
    m1.update(conv_row0=H, conv_T=T, c_row0=padL + 4)         # t: its history in rows [4, 4 + padL) of every stream
    m1["c_rows_b"] = m1["c_row0"] + T + 3
    X = m1["A"]
    ap = V.split_bits(R.silu(X, F32), npl)                    # [npl, B, rows, C]
    ap[:, :, H:H + T] = V.SENT_P                              # the new rows are the conversion's
    t_hist = V.garbage((B, m1["c_rows_b"], C)).copy()
    t_hist[:, 4:4 + padL] = np.random.default_rng(5000 + C).standard_normal((B, padL, C))
    cp = V.split_bits(t_hist, npl)
    cp[:, :, m1["c_row0"]:m1["c_row0"] + T] = V.SENT_P
    h1 = V.hook(m1, mode, ap.reshape(-1))
    h1["Cp"] = cp.reshape(-1).copy()
    h1["Cp_in"] = cp
    r = E.test_voc_conv([h1], C, mode, B, T, repeat=True)
    assert not r["refused"] and r["identical"] is True, K._last_error()
    got = h1["Ap"].reshape(ap.shape)
    new = np.zeros(m1["a_rows_b"], bool)
    new[H:H + T] = True
    _exact(name, "chain", np.array_equal(got[:, :, ~new], ap[:, :, ~new]), "input planes outside the converted rows unchanged")
    dec = got[:, :, new].view(np.float16).astype(F64)
    _exact(name, "chain", V.silu_planes_within_rounding(X[:, new], dec[0], dec[1] if npl == 2 else 0.0, npl), "SiLU'd input planes inside their rounding")
    out = h1["Cp"].reshape(cp.shape)
    wr = np.zeros(m1["c_rows_b"], bool)
    wr[m1["c_row0"]:m1["c_row0"] + T] = True
    _exact(name, "chain c1", np.array_equal(out[:, :, ~wr], cp[:, :, ~wr]), "Cp outside the written rows unchanged")
    _verify(record_property, h1, mode, name, "chain c1", exact_split=False)
    # c2: Ap = c1's Cp, residual = X's new rows (the engine's r_off = H C over X's own stream stride)
    m2 = V.member(5200 + C, C, B, T, taps, dil, idx=2, bias=True, Cf=True, Cp=True, conv=0)
    m2.update(a_rows_b=m1["c_rows_b"], a_row0=m1["c_row0"] - padL, res=X.reshape(-1).copy(), r_off=H * C, r_bstride=m1["a_rows_b"] * C)
    h2 = V.hook(m2, mode, h1["Cp"])
    r = E.test_voc_conv([h2], C, mode, B, T, repeat=True)
    assert not r["refused"] and r["identical"] is True, K._last_error()
    _exact(name, "chain c2", np.array_equal(h2["Ap"], h1["Cp"]), "planes handed in come back unchanged")
    _verify(record_property, h2, mode, name, "chain c2", exact_split=False)


@inst
def test_to_planes_act_row_major_arm(C, mname, record_property):
    """to_planes_act_kernel with blocked = 0 on its own (the hook's conversion step): nb = 3 streams, row0 > 0, fewer rows than a stream holds.
    Without SiLU the planes are the CPU h3_split exactly, with it inside the bound derived for the producer's silu_f; every other row keeps its bits"""
    mode, T = V.MODES[mname], V.TILE[C]
    npl, B = V.n_planes(mode), 3
    for conv in (1, 2):
        kernel, tag = "to_planes_act row-major " + mname, "C=%d silu=%d" % (C, conv - 1)
        m = V.member(6000 + C + conv, C, B, T, 1, 1, idx=1, bias=True, Cf=True, conv=conv)
        m.update(conv_row0=2, conv_T=T + 5)                    # rows [2, T + 7) of the T + 11 of a stream; the conv reads [5, 5 + T)
        assert m["a_row0"] == 5 and m["a_rows_b"] == T + 11
        m["A"] = (np.random.default_rng(6100 + C).standard_normal((B, m["a_rows_b"], C)) * 3.0).astype(F32)
        m["A"][0, 3, :4] = (0.0, -0.0, 6e-8, -30.0)            # zeros, an fp16 subnormal, a SiLU below the fp16 range
        h = V.hook(m, mode)
        r = K._E().test_voc_conv([h], C, mode, B, T)
        assert not r["refused"], K._last_error()
        P = h["Ap"].reshape(npl, B, m["a_rows_b"], C)
        done = np.zeros(m["a_rows_b"], bool)
        done[2:T + 7] = True
        _exact(kernel, tag, bool((P[:, :, ~done] == V.SENT_P).all()), "rows outside [row0, row0 + T) unchanged")
        if conv == 1:
            _exact(kernel, tag, np.array_equal(P[:, :, done], V.split_bits(m["A"][:, done], npl)), "planes equal the CPU h3_split")
        else:
            dec = P[:, :, done].view(np.float16).astype(F64)
            _exact(kernel, tag, V.silu_planes_within_rounding(m["A"][:, done], dec[0], dec[1] if npl == 2 else 0.0, npl), "planes of silu(x) inside their rounding")
        _verify(record_property, h, mode, _name(C, mname), "after to_planes_act silu=%d" % (conv - 1), exact_split=False)


@inst
def test_overflow_word(C, mname):
    """one input value beyond the fp16 range (7e4: its plane is inf) makes an output non-finite: the kernel sets its ovf word, as the planes GEMM does
    (test_fp16_planes_range_check_reports_an_operand_beyond_the_fp16_range); a clean input leaves it 0"""
    mode, T = V.MODES[mname], V.TILE[C]
    for bad in (False, True):
        ms = V.group(7000 + C, C, 3, T, (3, 7), (1, 3), "c2")
        if bad:
            ms[1]["A"][2, ms[1]["a_row0"] + 40, 3] = 7e4
        hs = [V.hook(m, mode) for m in ms]
        ovf = np.zeros(1, np.int32)
        r = K._E().test_voc_conv(hs, C, mode, 3, T, ovf=ovf)
        assert not r["refused"], K._last_error()
        assert int(ovf[0]) == (1 if bad else 0)
        assert np.isfinite(hs[0]["Cf"]).all() and bool(np.isfinite(hs[1]["Cf"]).all()) != bad


@inst
def test_refusals_write_nothing(C, mname):
    """what launch_voc_conv refuses, and rows outside the arrays (the hook's own check: nothing is launched): code 1, every output array and the
    overflow word as they went in"""
    mode, tile = V.MODES[mname], V.TILE[C]
    E = K._E()

    def group(taps=(3, 7), dils=(1, 3), T=tile, ch=C):
        return V.group(8000 + ch, ch, 2, T, taps, dils, "c2")

    def refused(ms, mode=mode, n=None, **over):
        hs = [V.hook(m, mode if mode in (V.H3, V.H1) else V.H1) for m in ms]
        for h in hs:
            h.update(over)
        before = [{k: h[k].copy() for k in ("Ap", "Wp", "Cf", "Cp", "res")} for h in hs]
        ovf = np.zeros(1, np.int32)
        r = E.test_voc_conv(hs, ms[0]["C"], mode, ms[0]["B"], ms[0]["T"], ovf=ovf, n=n)
        return r["refused"] and int(ovf[0]) == 0 and all(np.array_equal(h[k], b[k]) for h, b in zip(hs, before) for k in b)

    assert not refused(group())                                                    # the group as it is runs
    # the launcher's own refusals
    assert refused(group(ch=64))                                                   # C = 64
    assert refused(group(T=tile + 64)) and refused(group(T=tile // 2))             # T not a whole number of tiles
    assert refused(group(taps=(3, 12), dils=(1, 2)))                               # taps = 12
    assert refused(group(taps=(3, 4), dils=(1, 17)))                               # halo 51
    assert not refused(group(taps=(3, 3), dils=(1, 25)))                           # (halo 50 runs)
    assert refused(group(taps=(3, 7, 11), dils=(1, 3, 5)), n=4) and refused(group(), n=0)
    assert refused(group(), mode=0)                                                # the bf16 planes format
    assert refused(group(), drop=1) and refused(group(), drop=2)                   # a member without Ap / without Wp
    # rows outside the arrays, one condition at a time; member 0 (taps 3, dilation 1) is the one that leaves its arrays
    m0 = group()[0]
    assert refused(group(), a_row0=-1)
    assert refused(group(), a_rows_b=m0["a_row0"] + tile + 2 - 1)                  # one input row short
    assert refused(group(), c_row0=-1)
    assert refused(group(), c_row0=m0["c_rows_b"] - tile + 1)                      # the last Cp row one past the planes
    assert refused(group(), c_off=-4)
    assert refused(group(), c_off=m0["f_len"] - m0["c_bstride"] - tile * C + 4)    # the last Cf row four floats past the array
    assert refused(group(), r_off=-4)
    assert refused(group(), r_off=m0["res"].size - m0["r_bstride"] - tile * C + 4)
    assert refused(group(), conv_row0=-1) and refused(group(), conv_T=m0["a_rows_b"] + 1)
