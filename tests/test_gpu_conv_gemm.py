"""The conv-GEMM families in their CONV and EPILOGUE forms against float64 (tests/kernel_refs.py: conv_gemm), through the production path
(sva_test_conv_gemm: launch_conv_gemm_group for the dispatcher, launch_conv_gemm_group_plan for one given plan).  test_gpu_parity.py pins the
dense product C = A W^T + bias of every plan; here every plan meets taps over shifted rows with dilation and stride, padded A / C / residual
geometry, unstored rows, every epilogue stage, the prologues, groups of three and the XCD tile remap -- and the persistent LDS-DMA planes
kernel meets its conv form.  Cases, plans and the restated plan check live in tests/conv_gemm_cases.py (checked on the CPU by
tests/test_kernel_refs.py).

Bound (tests/test_gpu_kernels.py: _check): err <= 4 e32 + 4 ulp32(max |ref|) + extra, e32 from the float32 restatement of the same case.
extra = 0 for the f32-MFMA kernels (SmallM, Tiled, Ring, Stream); for Split the dropped bf16 part products (Member.split_extra); for the planes
kernel in H3 the dropped lo x lo product, and for an output that leaves as planes the output split's own rounding -- derived next to the case.
No bound of a linear-epilogue case may exceed the (8e-6 sqrt(K) + 1e-5) max |ref| of test_every_gemm_dispatch_choice_vs_fp64: a derived bound
above that ceiling fails the test as a wrong derivation.  No planes bound exceeds the 3e-6 (H3) / 2e-3 (H1) relative of
test_planes_gemm_every_mode_vs_fp64: it caps the derived one.
Exact: every element of C (and Cp) outside the stored ones -- pad columns, the c_off prefix, skipped rows, the tails between items -- keeps the
value it went in with; a refused plan returns the hook's "refused" code and leaves C alone; a repeated launch is bit-identical.

The activation pass that makes the A planes (to_planes_act_kernel) is reached here in its K-blocked arm only (blocked = 1, one stream, row 0); its
row-major arm, several streams and a first row > 0 are test_gpu_voc_conv.py: test_to_planes_act_row_major_arm.

With SVA_CONV_GEMM_PARITY_TABLE=<path> the run writes its table there (profiles/conv_gemm_parity.txt): one row per (family, shape, form) with
the family's worst plan; every plan's own error, bound and ratio are printed by the run and recorded as pytest properties."""
import os
import time

import numpy as np
import pytest

import conv_gemm_cases as G
import kernel_refs as R
import test_gpu_kernels as K

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    t0 = time.time()
    yield
    path = os.environ.get("SVA_CONV_GEMM_PARITY_TABLE")
    if path and _TABLE:
        # one row per (family, shape, form): the family's plans collapsed onto the one with the worst err / bound (every plan's own figures are
        # printed by the run and recorded as pytest properties), with the counts of plans compared, plans refused and exact checks that held
        rows = {}
        for kernel, tag, exact, err, bnd, ratio in _TABLE:
            r = rows.setdefault((_family(kernel), tag), dict(ran=0, refused=0, exact=0, worst=None))
            if not exact:
                r["ran"] += 1
                if r["worst"] is None or ratio > r["worst"][3]:
                    r["worst"] = (kernel, err, bnd, ratio)
            elif ratio == 0.0:
                r["refused" if exact.startswith("refused") else "exact"] += 1
            else:
                r["worst"] = (kernel + " " + exact, 1.0, 0.0, float("inf"))
        floats = [t for t in _TABLE if not t[2]]
        with open(path, "w") as f:
            f.write("# %d cases (%d compared with float64, %d exact checks), worst err / bound = %.3f, wall %.1f s\n" %
                    (len(_TABLE), len(floats), len(_TABLE) - len(floats), max(t[5] for t in _TABLE), time.time() - t0))
            f.write("%-14s %-34s %5s %7s %5s  %-30s %11s %11s %6s\n" % ("family", "shape form", "plans", "refused", "exact", "worst plan", "max_err", "bound", "ratio"))
            for (fam, tag), r in rows.items():
                k, e, b, q = r["worst"] or ("-", 0.0, 0.0, 0.0)
                f.write("%-14s %-34s %5d %7d %5d  %-30s %11.4e %11.4e %6.3f\n" % (fam, tag, r["ran"], r["refused"], r["exact"], k, e, b, q))


def _family(kernel):
    """'SmallM 1,4,1,z2' -> 'SmallM'; 'Stream 1,4,1,z1 Wk' -> 'Stream Wk'; 'PlanesDma 9 H3' -> 'PlanesDma H3'; the dispatcher's runs keep one name"""
    w = kernel.split()
    return "dispatcher" if w[0] == "dispatcher" else " ".join([w[0]] + [x for x in w[2:] if x in ("Wk", "H3", "H1")])


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


def _launch(members, plan, repeat=False, extras=None):
    hooks = [m.hook(**((extras or [{}] * len(members))[i])) for i, m in enumerate(members)]
    r = K._E().test_conv_gemm(hooks, plan, repeat=repeat)
    return r, hooks


def _untouched(m, Cout, keep):
    mask = np.ones(m.c_len, bool)
    mask[m.cidx[keep]] = False
    return np.array_equal(Cout[mask], m.C0[mask])


def _verify(record_property, m, Cout, name, tag, linear, extra=0.0):
    """stored elements against float64 under the derived bound, everything else in C exactly as it went in"""
    keep = m.stored()
    r64, r32 = m.ref(F64)[keep], m.ref(F32)[keep]
    ceil = None
    if linear:
        ceil = G.ceiling(m.K, r64)
        assert R.bound(R.e32_of(r32, r64), r64, extra) <= ceil, (name, tag, "derived bound above the dense-form ceiling")
    _check(record_property, name, tag, Cout[m.cidx][keep], r64, r32, extra=extra, ceiling=ceil)
    _exact(name, tag, _untouched(m, Cout, keep), "pad columns, c_off prefix, skipped rows and item tails unchanged")


def _extra(fam, m):
    return m.split_extra() if fam == G.SPLIT else 0.0


def _run_plans(record_property, m, shape, form, plans, wk=False, repeat=False):
    P, linear = m.problem(), form in G.LINEAR_FORMS
    ran = 0
    for plan in plans:
        name, tag = G.plan_name(plan) + (" Wk" if wk else ""), "%s %s" % (shape, form)
        r, hooks = _launch([m], plan, repeat=repeat, extras=[dict(use_wk=1)] if wk else None)
        if not G.plan_accepts(plan, P):
            _exact(name, tag, r["refused"] and np.array_equal(hooks[0]["C"], m.C0), "refused, C untouched")
            continue
        assert not r["refused"], (name, tag, K._last_error())
        assert r["kind"] == G.REPORT_KIND[plan[0]]
        _verify(record_property, m, hooks[0]["C"], name, tag, linear, _extra(plan[0], m))
        if repeat:
            _exact(name, tag, r["identical"] is True, "second launch bit-identical")
        ran += 1
    return ran


def _run_dispatcher(record_property, members, shape, form, operands=0, pmode=-1, extras=None, cp_silu=False):
    """kind = -1: what runs is what sva_test_gemm_plan answers for the same descriptor on the CPU"""
    r, hooks = _launch(members, None, extras=extras)
    assert not r["refused"], (shape, form, K._last_error())
    want = K._E().test_gemm_plan([m.plan_desc(operands, pmode, cp_silu) for m in members])
    assert r["kind"] == want[5], (shape, form, r["kind"], want)
    return want, hooks


# =====================================================================================================================================
# fp32 families
# =====================================================================================================================================
@pytest.mark.parametrize("form", list(G.FORMS))
def test_every_plan_every_epilogue_form(form, record_property):
    """one epilogue form on its shape (P0; E7 on its taps = 1 twin, E8 on the 14-row ConvNeXt shape) through every plan of every fp32 family, the
    weight-streaming kernel on row-major and on fragment-major weights, and once through the dispatcher"""
    shape = G.shape_of(form)
    m = G.case(shape, form)
    ran = _run_plans(record_property, m, shape, form, G.ALL_PLANS)
    ran += _run_plans(record_property, m, shape, form, G.STREAM_PLANS, wk=True)
    by_family = {f: sum(1 for p in G.ALL_PLANS if p[0] == f and G.plan_accepts(p, m.problem())) for f in (G.SMALLM, G.TILED, G.RING, G.SPLIT, G.STREAM)}
    for f, cnt in by_family.items():
        assert (cnt == 0) == ((f, form) in G.REFUSED_BY_DESIGN), (G.FAMILY_NAME[f], form, cnt)
    assert ran >= 3
    want, hooks = _run_dispatcher(record_property, [m], shape, form)
    _verify(record_property, m, hooks[0]["C"], "dispatcher -> " + G.plan_name(want[:5]), "%s %s" % (shape, form), form in G.LINEAR_FORMS, _extra(want[0], m))


@pytest.mark.parametrize("form", ["E0", "E2"])
def test_grid_level_k_split_plans_twice(form, record_property):
    """the small-M kernel with its K axis also split over z = 2 / 4 / 8 workgroups: the last arriver sums the partials in split order and re-arms
    the tile's counter, so a second launch from the same C must give the same bits"""
    m = G.case("P0", form)
    assert _run_plans(record_property, m, "P0", form, G.SKINNY_Z, repeat=True) == 21          # (N = 136 takes one column tile per wave: 7 plans x 3 splits)
    m = G.case("P0w", form)                 # two and four column tiles per wave: N = 128
    assert _run_plans(record_property, m, "P0w", form, G.SKINNY_Z, repeat=True) == 60
    want, hooks = _run_dispatcher(record_property, [m], "P0w", form)
    _verify(record_property, m, hooks[0]["C"], "dispatcher -> " + G.plan_name(want[:5]), "P0w %s" % form, True, _extra(want[0], m))


@pytest.mark.parametrize("shape,form", [("P0s", "E0"), ("P0s", "E2"), ("P1", "E0"), ("P1", "E3"), ("P1n", "E0"), ("P1n", "E3"), ("P0w", "E1"), ("P0w", "E2"),
                                        ("P0w", "E4"), ("P0", "E5w")])
def test_every_plan_other_conv_shapes(shape, form, record_property):
    """the downsampling form (stride 2, four taps), the narrow HiFiGAN level (seven taps at dilation 3; N = 32 and N = Cin = 16: the tiled
    variants for narrow outputs, the 16-deep K tile), and P0 at N = 128 / SwiGLU at N = 192 (N = 136 only ever takes ONE column tile per small-M
    wave: here two and four) through every plan that takes them -- the others must refuse"""
    m = G.case(shape, form)
    ran = _run_plans(record_property, m, shape, form, G.ALL_PLANS)
    ran += _run_plans(record_property, m, shape, form, G.STREAM_PLANS, wk=True)
    assert ran >= 20
    want, hooks = _run_dispatcher(record_property, [m], shape, form)
    _verify(record_property, m, hooks[0]["C"], "dispatcher -> " + G.plan_name(want[:5]), "%s %s" % (shape, form), form in G.LINEAR_FORMS, _extra(want[0], m))


def test_xcd_tile_remap_with_a_ragged_tile_count(record_property):
    """PX: 1093 rows x 136 columns.  The tiled kernel's 64 x 64 and 64 x 128 tiles give 3 x 18 = 54 and 2 x 18 = 36 tiles: xcd_swizzle_for (nx >= 2,
    ny >= 16) turns the XCD remap on with a tile count that is no multiple of 8, so the uneven bands of xcd_tile are walked.  The committed policy
    itself sends a single problem (and a group) of this size to the small-M kernel, which has no remap: the dispatcher run below checks that choice."""
    m = G.case("PX", "E0")
    for plan, (bm, bn) in (((G.TILED, 0, 0, 0, 1), (64, 64)), ((G.TILED, 5, 0, 0, 1), (64, 128))):
        nx, ny = -(-m.N // bn), -(-m.M // bm)
        assert nx >= 2 and ny >= 16 and (nx * ny) % 8 != 0
        assert _run_plans(record_property, m, "PX", "E0", [plan]) == 1
    want, hooks = _run_dispatcher(record_property, [m], "PX", "E0")
    _verify(record_property, m, hooks[0]["C"], "dispatcher -> " + G.plan_name(want[:5]), "PX E0", True, _extra(want[0], m))


GROUP_PLANS = {"P1": [(G.SMALLM, 1, 4, 1, 1), (G.SMALLM, 2, 8, 2, 1), (G.SMALLM, 4, 4, 2, 1), (G.TILED, 0, 0, 0, 1), (G.TILED, 2, 0, 0, 1), (G.SPLIT, 1, 0, 0, 1),
                      (G.SPLIT, 3, 0, 0, 1), (G.RING, 0, 0, 0, 1), (G.STREAM, 1, 4, 1, 1)],
               "P1w": [(G.RING, 0, 0, 0, 1), (G.RING, 6, 0, 0, 1), (G.SPLIT, 3, 0, 0, 1)]}


@pytest.mark.parametrize("form", ["E3", "E4"])
@pytest.mark.parametrize("shape", ["P1", "P1w"])
def test_groups_of_three_branches(shape, form, record_property):
    """the three ResBlock branches of a HiFiGAN level -- taps (3, 7, 11) at dilations (1, 3, 5), separate A / W / bias / C -- as ONE launch, through
    the dispatcher and through given plans (P1w: P1 with the 64 channels the ring kernel needs; on P1 the ring and the weight-streaming kernel must
    refuse: Cin = 32, single problems only).  Each member against its own reference; the same group with its members permuted gives every member
    the same bits."""
    ms = [G.case(shape, form, taps=t, dil=d) for t, d in ((3, 1), (7, 3), (11, 5))]
    P = max(ms, key=lambda m: m.taps).problem()
    tag = "%s %s x3" % (shape, form)
    want, hooks = _run_dispatcher(record_property, ms, shape, form)
    for i, m in enumerate(ms):
        _verify(record_property, m, hooks[i]["C"], "dispatcher -> " + G.plan_name(want[:5]), tag + " #%d" % i, True, _extra(want[0], m))
    ran = 0
    for plan in GROUP_PLANS[shape]:
        name = G.plan_name(plan)
        r, hooks = _launch(ms, plan)
        if not G.plan_accepts(plan, P, n=3):
            _exact(name, tag, r["refused"] and all(np.array_equal(h["C"], m.C0) for h, m in zip(hooks, ms)), "refused, C untouched")
            continue
        assert not r["refused"], (name, tag, K._last_error())
        for i, m in enumerate(ms):
            _verify(record_property, m, hooks[i]["C"], name, tag + " #%d" % i, True, _extra(plan[0], m))
        perm = (2, 0, 1)
        r2, hooks2 = _launch([ms[j] for j in perm], plan)
        assert not r2["refused"]
        _exact(name, tag, all(np.array_equal(hooks2[k]["C"], hooks[j]["C"]) for k, j in enumerate(perm)), "members permuted: bit-identical per member")
        ran += 1
    assert ran >= 3


def test_refusals_of_fields_a_kernel_does_not_implement():
    """plan_accepts refuses what a family's kernel would silently drop: the tiled kernel with rms_w / dw_wT (it ran and returned the un-normalised
    product); SwiGLU on the tiled 256 x 16 tile (a pair does not fit: it read past the tile) and on one column tile per small-M wave (it stored
    nothing); the small-M ConvNeXt prologue beyond one 16 x 16 tile, with more than 16 rows or together with SiLU; the fused RMSNorm together with
    SiLU on load (SiLU was dropped) or with taps (the statistic ran over taps x Cin values).  C comes back untouched."""
    E = K._E()

    def refused(m, plan, **extra):
        h = m.hook(**extra)
        r = E.test_conv_gemm([h], plan)
        return r["refused"] and np.array_equal(h["C"], m.C0)

    m7, m8, m5 = G.case("P0t1", "E7"), G.case("PD", "E8"), G.case("P0", "E5")
    for v in range(8):
        assert refused(m7, (G.TILED, v, 0, 0, 1)) and refused(m8, (G.TILED, v, 0, 0, 1))
    assert refused(m5, (G.TILED, 3, 0, 0, 1)) and refused(m5, (G.SMALLM, 1, 4, 1, 1)) and refused(m5, (G.STREAM, 1, 4, 1, 1))
    for plan in ((G.SMALLM, 2, 4, 1, 1), (G.SMALLM, 1, 4, 2, 1), (G.SMALLM, 4, 8, 4, 1)):
        assert refused(m8, plan)
    assert refused(m8, (G.SMALLM, 1, 4, 1, 1), a_silu=1)
    big = G.Member(np.random.default_rng(3), dict(G.SHAPES["PD"], T=9), "E8")            # M = 18 > 16
    assert refused(big, (G.SMALLM, 1, 4, 1, 1))
    assert refused(m7, (G.SMALLM, 1, 4, 1, 1), a_silu=1) and refused(m7, (G.RING, 0, 0, 0, 1), a_silu=1) and refused(m7, (G.STREAM, 1, 4, 1, 1), a_silu=1)
    taps3 = G.Member(np.random.default_rng(4), "P0", "E7")                               # rms_w with three taps
    for plan in ((G.SMALLM, 1, 4, 1, 1), (G.RING, 0, 0, 0, 1), (G.STREAM, 1, 4, 1, 1)):
        assert refused(taps3, plan)
    # and the dispatcher refuses the same problems
    for m, extra in ((taps3, {}), (big, {}), (m7, dict(a_silu=1))):
        h = m.hook(**extra)
        assert E.test_conv_gemm([h], None)["refused"] and np.array_equal(h["C"], m.C0)


# =====================================================================================================================================
# planes kernel, conv form (the persistent LDS-DMA kernel: taps over A planes, a group's tiles as one sequence, SiLU'd output planes)
# =====================================================================================================================================
PL_FORMS = {"bias": dict(bias=True), "bias+res": dict(bias=True, res=True), "bias+res+acc": dict(bias=True, res=True, accumulate=True, scale=float(F32(1.0) / F32(3.0)))}
WP, AP, CP = 8, 16, 32
_PL = {}


def _pl_member(Cin, N, form, taps, dil):
    """PL: B = 2, T = 150 (M = 300: a ragged third 128-row tile), A over dense rows of Cin values"""
    key = (Cin, N, form, taps, dil)
    if key not in _PL:
        shape = dict(B=2, T=150, Cin=Cin, taps=taps, dil=dil, stride=1, N=N, lda=Cin, ldc=N, c_off=N)
        _PL[key] = G.Member(np.random.default_rng(500 + Cin + N + 13 * taps + len(form)), shape, PL_FORMS[form], dense=True)
    return _PL[key]


def _pl_operands(m, mode, Ap, silu):
    """the operands AS THE PLANES HOLD THEM, restated from planes_split.h / make_weight_planes: (A rows fp64, A lo rows, W fp64, |W lo|).  Without
    SiLU the A planes must equal the CPU split of A exactly; with it (the producer's fast exp) they are taken from the device and must sit within
    the planes' own rounding of silu(A): half an fp16 ulp (H1, 2^-11) / the lo plane's half ulp (H3, 2^-22), plus the float32 error of silu_f (derived below) and 2^-24
    absolute for fp16 subnormals"""
    npl = 2 if mode == 1 else 1
    rows_n = m.A.size // m.Cin
    Ap = Ap.reshape(npl, -1)
    hi = R.planes_decode(Ap[:1], 1, rows_n, m.Cin, True).reshape(-1)
    lo = R.planes_decode(Ap[1:], 1, rows_n, m.Cin, True).reshape(-1) if npl == 2 else np.zeros_like(hi)
    if not silu:
        chi, clo = R.h3_split(m.A)
        assert np.array_equal(hi, chi.astype(F64)) and (npl == 1 or np.array_equal(lo, clo.astype(F64))), "A planes differ from the CPU split"
    else:
        # the producer's silu_f(x) = x / (1 + __expf(-x)) in float32: the intrinsic is exp2(-x log2 e), whose argument product rounds once
        # (2^-24 |x| relative in e = exp(-x)) before a 1-ulp exp2; e enters silu with sensitivity e / (1 + e) <= min(1, e); the add and the
        # division round once each and the division may be 2 ulp off: min(1, e) (|x| + 1) 2^-24 + 4 2^-24 relative
        x = m.A.astype(F64)
        s = R.silu(x)
        with np.errstate(over="ignore"):
            dev = (np.minimum(1.0, np.exp(-x)) * (np.abs(x) + 1.0) + 4.0) * 2.0 ** -24
        rel = 2.0 ** -11 if npl == 1 else 2.0 ** -22
        assert (np.abs(hi + lo - s) <= (rel + dev) * np.abs(s) + 2.0 ** -24).all(), "SiLU'd A planes outside their rounding"
    whi, wlo = R.weight_planes(m.W, npl)
    return hi + lo, lo, whi + wlo, np.abs(wlo)


def _pl_verify(record_property, m, h, mode, silu, name, tag, cp_silu=False):
    a, alo, w, wlo = _pl_operands(m, mode, h["Ap"], silu)
    key = ("pl", mode, silu)
    rows = m.rows(A=a)
    r64, r32 = m.ref(F64, rows=rows, W=w, key=key), m.ref(F32, rows=rows.astype(F32), W=w.astype(F32), key=key)
    # H3 computes hi hi + hi lo + lo hi: the dropped lo x lo product, through the epilogue's gain (|scale| here); H1 drops nothing of what it holds
    extra = 0.0
    if mode == 1:
        extra = float((np.abs(m.rows(A=alo)).reshape(m.M, m.K) @ wlo.T).max()) * abs(m.scale)
    rel = 3e-6 if mode == 1 else 2e-3          # the dense planes test's bound caps the derived one (the naive float32 sum over K = 704 alone passes it in H3)
    keep = m.stored()
    _check(record_property, name, tag, h["C"][m.cidx][keep], r64[keep], r32[keep], extra=extra, ceiling=rel * float(np.abs(r64[keep]).max()))
    _exact(name, tag, _untouched(m, h["C"], keep), "pad rows and item tails of C unchanged")
    if cp_silu:
        # Cp = planes of silu(v): the kernel's v within `vb` of the reference moves silu by at most 1.1 vb; the output split rounds once more --
        # one fp16 ulp of the value in H1 (2^-10), 2^-22 in H3, 2^-24 absolute in the subnormal range
        npl = 2 if mode == 1 else 1
        cp_rows = m.c_len // m.ldc
        got = R.planes_decode(h["Cp"].reshape(npl, -1), npl, cp_rows, m.N, True)
        rowidx = m.cidx[:, :, 0] // m.ldc
        s64, s32 = R.silu(r64), R.silu(r32, F32)
        rnd = (2.0 ** -10 if mode == 2 else 2.0 ** -22) * float(np.abs(s64).max()) + 2.0 ** -24
        _check(record_property, name, tag + " Cp", got[rowidx], s64, s32, extra=1.1 * extra + rnd, ceiling=rel * float(np.abs(s64).max()))
        mask = np.ones(cp_rows, bool)
        mask[rowidx.reshape(-1)] = False
        sent = np.full((npl, cp_rows * m.N), 0x3555, np.uint16)
        sent_rows = R.planes_decode(sent, npl, cp_rows, m.N, True)
        _exact(name, tag, np.array_equal(got[mask], sent_rows[mask]), "pad rows of Cp unchanged")


@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("mode", [1, 2], ids=["H3", "H1"])
def test_planes_dma_conv_form(mode, Cin, record_property):
    """variants 9 / 10 / 11 (128 x 128 tiles, N = 128) and 13 / 14 (narrow tiles, N = 64): a single conv problem, the three-branch group with bias +
    residual, the same group accumulating, SiLU'd output planes beside C, and A planes built with SiLU; every launch twice, bit-identical (a hazard
    in the persistent pipeline shows up as a rare wrong tile).  Reference: float64 on the operands as the planes hold them."""
    E = K._E()
    npl = 2 if mode == 1 else 1
    branches = ((3, 1), (7, 3), (11, 5))
    for variant in (9, 10, 11, 13, 14):
        N = 128 if variant <= 11 else 64
        plan = (G.PLANESDMA, variant, 0, 0, 1)
        name = "PlanesDma %d %s" % (variant, "H3" if mode == 1 else "H1")
        cases = [("single", [_pl_member(Cin, N, "bias", 3, 2)], 1, False), ("group", [_pl_member(Cin, N, "bias+res", t, d) for t, d in branches], 1, False),
                 ("group acc", [_pl_member(Cin, N, "bias+res+acc", t, d) for t, d in branches], 1, False),
                 ("cp_silu", [_pl_member(Cin, N, "bias", 3, 2)], 1, True), ("silu A", [_pl_member(Cin, N, "bias+res", 3, 2)], 2, False)]
        for what, ms, a_planes, cp_silu in cases:
            tag = "PL Cin=%d N=%d %s" % (Cin, N, what)
            extras = []
            for m in ms:
                x = dict(pmode=mode, a_planes=a_planes, Ap=np.zeros(npl * m.A.size, np.uint16))
                if cp_silu:
                    x.update(c_planes=1, cp_silu=1, Cp=np.full(npl * (m.c_len // m.ldc) * m.N, 0x3555, np.uint16))
                extras.append(x)
            r, hooks = _launch(ms, plan, repeat=True, extras=extras)
            assert not r["refused"], (name, tag, K._last_error())
            for i, m in enumerate(ms):
                _pl_verify(record_property, m, hooks[i], mode, a_planes == 2, name, tag + (" #%d" % i if len(ms) > 1 else ""), cp_silu)
            _exact(name, tag, r["identical"] is True, "second launch bit-identical")
            if variant == 9:        # the dispatcher's own variant for the same problem
                r, hooks = _launch(ms, None, extras=extras)
                want = E.test_gemm_plan([m.plan_desc(WP | AP | (CP if cp_silu else 0), mode, cp_silu) for m in ms])
                assert not r["refused"] and r["kind"] == want[5] and want[0] == G.PLANESDMA, (tag, r, want)
                for i, m in enumerate(ms):
                    _pl_verify(record_property, m, hooks[i], mode, a_planes == 2, "dispatcher -> PlanesDma %d" % want[1], tag + (" #%d" % i if len(ms) > 1 else ""), cp_silu)
    # variant 12 takes no conv form; the register-staged variants take no taps over A planes
    m = _pl_member(Cin, 128, "bias", 3, 2)
    for plan in ((G.PLANESDMA, 12, 0, 0, 1), (G.PLANES, 0, 0, 0, 1)):
        h = m.hook(pmode=mode, a_planes=1)
        assert E.test_conv_gemm([h], plan)["refused"] and np.array_equal(h["C"], m.C0)
    # operands that exist only as planes (A null / C null) are the planes kernel's: every plan of every fp32 family must refuse them
    P = dict(m.problem(), planes=True)
    for plan in G.ALL_PLANS + G.SKINNY_Z[:3]:
        assert not G.plan_accepts(plan, P)
        for x in (dict(a_planes=1), dict(c_planes=2, Cp=np.full(npl * (m.c_len // m.ldc) * m.N, 0x3555, np.uint16))):
            h = m.hook(pmode=mode, **x)
            _exact(G.plan_name(plan), "PL Cin=%d N=128 %s only" % (Cin, "Ap" if "a_planes" in x else "Cp"),
                   E.test_conv_gemm([h], plan)["refused"] and np.array_equal(h["C"], m.C0), "refused, C untouched")
