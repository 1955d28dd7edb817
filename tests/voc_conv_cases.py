"""Cases and the comparison rule of the voc_conv_kernel tests (tests/test_gpu_voc_conv.py), importable without a GPU: tests/test_kernel_refs.py runs
the rule on reference-versus-mutated-reference at the same shapes, so that the rule is known to bite.

A member is one branch of a conv stage (csrc/sva_common.h: VocConv) as the dict the hook takes (engine.test_voc_conv), with geometry fields that
all differ from each other inside a case -- a_rows_b / c_rows_b, a_row0 / c_row0, c_off / r_off, the strides -- so that no field can stand in for
another.  Input rows that no tap may read (in front of a_row0, behind a_row0 + T + padL - 1) hold +-1e4: one row too early or too late dominates.
Outputs go in filled with sentinels (SENT / 0x3555).

Rule (tests/test_gpu_conv_gemm.py: _pl_verify, unchanged): float64 on the operands as the planes hold them; err <= 4 e32 + 4 ulp32 + extra, extra =
the dropped lo x lo product in H3 and 0 in H1, capped by 3e-6 (H3) / 2e-3 (H1) of max |ref|; the SiLU'd output planes with extra = 1.1 extra + the
output split's own rounding (2^-22 H3 / 2^-10 H1 of max |silu| + 2^-24)."""
import numpy as np

import kernel_refs as R

F32, F64 = np.float32, np.float64
H3, H1 = 1, 2
MODES = {"H3": H3, "H1": H1}
SENT, SENT_P = F32(777.0), 0x3555
TILE = {32: 128, 16: 256}                # output rows per tile of the kernel's two instantiations per mode
REL = {H3: 3e-6, H1: 2e-3}               # the ceilings of test_planes_gemm_every_mode_vs_fp64
RES_K, RES_D = (3, 7, 11), (1, 3, 5)     # the engine's ResBlock taps and dilations
FORMS = {"c1": dict(bias=True, Cp=True), "c2": dict(bias=True, res=True, Cf=True, Cp=True), "c2 last": dict(bias=True, res=True, Cf=True)}


def n_planes(mode):
    return 2 if mode == H3 else 1


def padded_k(C, taps):
    """K of the weight planes: taps C, at C = 16 padded to whole 32-k blocks (csrc/sva_common.h: padded_weight_k)"""
    return taps * C if C != 16 else (taps * C + 31) // 32 * 32


def garbage(shape):
    """+-1e4 in a checkerboard (finite in fp16, and exact there)"""
    r, c = np.indices(shape[-2:])
    return np.broadcast_to(np.where((r + c) % 2 == 0, 1e4, -1e4), shape).astype(F32)


def member(seed, C, B, T, taps, dil, idx=0, bias=False, res=False, Cf=False, Cp=False, conv=1):
    """the hook's dict for one member, arrays included.  idx staggers the geometry inside a group"""
    rng = np.random.default_rng(seed)
    padL = (taps - 1) * dil
    m = dict(C=C, B=B, T=T, taps=taps, dil=dil)
    m["a_row0"] = 3 + 2 * idx
    m["a_rows_b"] = m["a_row0"] + T + padL + 5 + idx
    A = garbage((B, m["a_rows_b"], C)).copy()
    A[:, m["a_row0"]:m["a_row0"] + T + padL] = rng.standard_normal((B, T + padL, C)) * 1.5 + 0.1
    m["A"] = A
    m["conv"], m["conv_row0"], m["conv_T"] = conv, 0, m["a_rows_b"]          # the whole array becomes planes: the garbage rows too
    m["W"] = (rng.standard_normal((C, taps * C)) / np.sqrt(taps * C) + 0.01).astype(F32)
    if bias:
        m["bias"] = (rng.standard_normal(C) * 0.3).astype(F32)
    if res:
        m["r_off"] = C * (4 + idx) + 8
        m["r_bstride"] = m["r_off"] + T * C + 16 + 4 * idx
        m["res"] = rng.standard_normal(B * m["r_bstride"] + 12).astype(F32)
    if Cf:
        m["c_off"] = C * (1 + idx) + 4
        m["c_bstride"] = m["c_off"] + T * C + 8 + 4 * idx
        m["f_len"] = B * m["c_bstride"] + 20
    if Cp:
        m["c_row0"] = 7 + 3 * idx
        m["c_rows_b"] = m["c_row0"] + T + 2 + idx
    return m


def group(seed, C, B, T, taps, dils, form):
    return [member(seed + 17 * i, C, B, T, t, d, idx=i, **FORMS[form]) for i, (t, d) in enumerate(zip(taps, dils))]


def hook(m, mode, Ap=None):
    """a fresh launch of member m: its arrays with new output arrays full of sentinels (Ap: planes handed in ready, or the sentinel the conversion
    overwrites)"""
    npl = n_planes(mode)
    h = dict(m)
    h["Ap"] = np.full(npl * m["A"].size, SENT_P, np.uint16) if Ap is None else np.array(Ap, np.uint16)
    h["Wp"] = np.full(npl * m["C"] * padded_k(m["C"], m["taps"]), SENT_P, np.uint16)
    if "res" in m:
        h["res"], h["res_in"] = m["res"].copy(), m["res"]
    if "f_len" in m:
        h["Cf"] = np.full(m["f_len"], SENT, F32)
    if "c_rows_b" in m:
        h["Cp"] = np.full(npl * m["B"] * m["c_rows_b"] * m["C"], SENT_P, np.uint16)
    return h


def split_bits(x, npl):
    """the planes of fp32 values as uint16 bits [npl, ...] (planes_split.h on the CPU)"""
    hi, lo = R.h3_split(x)
    return np.stack([hi, lo][:npl]).astype(np.float16).view(np.uint16)


def res_rows(m):
    """[B, T, C] of the flat residual array"""
    B, T, C = m["B"], m["T"], m["C"]
    i = np.arange(B)[:, None] * m["r_bstride"] + m["r_off"] + np.arange(T * C)[None, :]
    return m["res"][i].reshape(B, T, C)


def cf_index(m):
    B, T, C = m["B"], m["T"], m["C"]
    return (np.arange(B)[:, None] * m["c_bstride"] + m["c_off"] + np.arange(T * C)[None, :]).reshape(B, T, C)


def cp_rows(m):
    """dense row numbers [B, T] of the output planes"""
    return np.arange(m["B"])[:, None] * m["c_rows_b"] + m["c_row0"] + np.arange(m["T"])[None, :]


def weight_exp(W):
    """e of make_weight_planes: max |W| 2^e in [2^7, 2^8)"""
    mx = float(np.abs(np.asarray(W, F32)).max())
    return 8 - int(np.frexp(F32(mx))[1]) if mx > 0 else 0


def cpu_operands(m, mode):
    """(a, |a lo|, w, |w lo|) as the planes hold them when the whole of A is split without SiLU: planes_split.h / make_weight_planes on the CPU"""
    npl = n_planes(mode)
    hi, lo = R.h3_split(m["A"])
    lo = lo.astype(F64) if npl == 2 else np.zeros(hi.shape)
    whi, wlo = R.weight_planes(m["W"], npl)
    return hi.astype(F64) + lo, np.abs(lo), whi + wlo, np.abs(wlo)


def reference(m, a, w, res=None, **over):
    """(v, silu v) in float64 and float32 on the given operands; `over` replaces geometry (the deliberate errors of the sensitivity test)"""
    g = dict(taps=m["taps"], dil=m["dil"], a_row0=m["a_row0"], T=m["T"])
    g.update(over)
    bias = m.get("bias")
    if res is None and "res" in m:
        res = res_rows(m)
    a = np.asarray(a, F64).reshape(m["B"], m["a_rows_b"], m["C"])
    v64, s64 = R.voc_conv_ref(a, w, bias, res, dt=F64, **g)
    v32, s32 = R.voc_conv_ref(a.astype(F32), np.asarray(w, F32), bias, res, dt=F32, **g)
    return v64, s64, v32, s32


def rule(m, mode, a, alo, w, wlo):
    """what the comparison needs: the references and, for the fp32 output and for the SiLU'd output planes, (extra, ceiling) of _check"""
    v64, s64, v32, s32 = reference(m, a, w)
    extra = 0.0
    if mode == H3:          # hi hi + hi lo + lo hi: the dropped lo x lo product
        lo3 = np.abs(np.asarray(alo, F64)).reshape(m["B"], m["a_rows_b"], m["C"])
        extra = float(R.voc_conv_ref(lo3, np.abs(wlo), None, None, m["taps"], m["dil"], m["a_row0"], m["T"])[0].max())
    rnd = (2.0 ** -10 if mode == H1 else 2.0 ** -22) * float(np.abs(s64).max()) + 2.0 ** -24
    return dict(v64=v64, v32=v32, s64=s64, s32=s32, extra=extra, ceiling=REL[mode] * float(np.abs(v64).max()), extra_p=1.1 * extra + rnd,
                ceiling_p=REL[mode] * float(np.abs(s64).max()))


def bound_of(f64, f32, extra, ceiling):
    """the bound _check applies: min(4 e32 + 4 ulp32(max |ref|) + extra, ceiling)"""
    return min(R.bound(R.e32_of(f32, f64), f64, extra), ceiling)


def silu_planes_within_rounding(x, hi, lo, npl):
    """planes of silu(x) made on the device (the producer's fast exp) against float64 -- the bound derived in test_gpu_conv_gemm.py (_pl_operands): the
    planes' own rounding (2^-11 H1 / 2^-22 H3) plus the float32 error of silu_f, min(1, e) (|x| + 1) 2^-24 + 4 2^-24 relative, plus 2^-24 absolute"""
    x = np.asarray(x, F64)
    s = R.silu(x)
    with np.errstate(over="ignore"):
        dev = (np.minimum(1.0, np.exp(-x)) * (np.abs(x) + 1.0) + 4.0) * 2.0 ** -24
    rel = 2.0 ** -11 if npl == 1 else 2.0 ** -22
    return bool((np.abs(np.asarray(hi, F64) + np.asarray(lo, F64) - s) <= (rel + dev) * np.abs(s) + 2.0 ** -24).all())
