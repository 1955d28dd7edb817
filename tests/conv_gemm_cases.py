"""Cases of tests/test_gpu_conv_gemm.py, built on the CPU: the shapes and epilogue forms, the operands with their padding, the plans of every
conv-GEMM family, a Python restatement of the plan check (csrc/gemm_dispatch.hip: plan_accepts and the *_supported predicates it calls) and the
table of (family, form) pairs that are refused by design.  tests/test_kernel_refs.py checks the table against the restatement without a GPU;
the GPU tests then require exactly that behaviour of the library: a refused plan returns the hook's "refused" code and leaves C alone, any
other plan runs."""
import numpy as np

import kernel_refs as R

F32, F64 = np.float32, np.float64
SENT = 777.0
PAD = 1e4                                   # every pad row / column of A is +-1e4: one wrong row or column dominates the sum

# GemmFamily (csrc/sva_common.h) and the family numbers of the profiling tables (plan_report_kind)
SMALLM, TILED, RING, SPLIT, F16W, STREAM, PLANES, PLANESDMA, STREAMH = range(9)
FAMILY_NAME = {SMALLM: "SmallM", TILED: "Tiled", RING: "Ring", SPLIT: "Split", STREAM: "Stream", PLANES: "Planes", PLANESDMA: "PlanesDma"}
REPORT_KIND = {SMALLM: 0, TILED: 1, RING: 2, SPLIT: 4, STREAM: 6}
FAMILY_OF_KIND = {v: k for k, v in REPORT_KIND.items()}

# ---- shapes: the smallest that cross every tile edge ------------------------------------------------------------------------------------------
# P0: M = 135 = one 128-row tile + 7, item boundaries at rows 45 and 90 inside a tile; K = 192 = 12 sixteen-blocks (fewer than 16 K-split waves);
#     N = 136: a multiple of 8, not of 16 / 64 / 128.  P0s: the downsampling form.  P1: a narrow HiFiGAN level, every 32-k block inside one tap;
#     P1n: 16 channels in and out (the K tile of 16, the tiled variant for N <= 16).  PX: 1093 rows x 136 columns in 64-row tiles = 18 x 3 tiles, so
#     the tiled kernels' XCD remap is on with a tile count (54) that is no multiple of 8.
SHAPES = {
    "P0": dict(B=3, T=45, Cin=64, taps=3, dil=2, stride=1, N=136, lda=80, ldc=140, c_off=4),
    "P0s": dict(B=3, T=45, Cin=64, taps=4, dil=1, stride=2, N=136, lda=80, ldc=140, c_off=4),
    "P0t1": dict(B=3, T=45, Cin=64, taps=1, dil=1, stride=1, N=136, lda=80, ldc=140, c_off=4),
    "P1": dict(B=2, T=150, Cin=32, taps=7, dil=3, stride=1, N=32, lda=36, ldc=36, c_off=4),
    "P1n": dict(B=2, T=150, Cin=16, taps=7, dil=3, stride=1, N=16, lda=20, ldc=20, c_off=4),
    "P1w": dict(B=2, T=150, Cin=64, taps=7, dil=3, stride=1, N=32, lda=68, ldc=36, c_off=4),       # P1 with the 64 channels the ring kernel needs
    "PX": dict(B=1, T=1093, Cin=16, taps=3, dil=1, stride=1, N=136, lda=20, ldc=140, c_off=4),
    "P0w": dict(B=3, T=45, Cin=64, taps=3, dil=2, stride=1, N=128, lda=80, ldc=132, c_off=4),       # P0 with N = 128: two and four column tiles per small-M wave
    "PD": dict(B=2, T=7, Cin=128, taps=1, dil=1, stride=1, N=136, lda=132, ldc=140, c_off=4),       # the ConvNeXt prologue: M = 14 <= 16
}
# ---- epilogue forms ---------------------------------------------------------------------------------------------------------------------------
FORMS = {
    "E0": dict(bias=True),
    "E1": dict(bias=True, act=1),
    "E2": dict(bias=True, gamma=True, res=True, skip=(20, 26)),
    "E3": dict(a_silu=True, bias=True, res=True),
    "E4": dict(accumulate=True, scale=float(F32(1.0) / F32(3.0))),
    "E5": dict(w13=True, N=160),
    "E6": dict(act=2, nonneg=True),
    "E7": dict(rms=True, bias=True),
    "E8": dict(dw=True, bias=True),
    "E9": dict(bias=True, ldc=137, c_off=1),
}
FORMS_MORE = {"E5w": dict(w13=True, N=192)}          # SwiGLU at N % 64 == 0: four column tiles per small-M wave (not one of the ten forms of the table above)
LINEAR_FORMS = ("E0", "E2", "E3", "E4", "E9")       # a linear epilogue: the ceiling of test_every_gemm_dispatch_choice_vs_fp64 applies


def ceiling(K, ref):
    return (8e-6 * np.sqrt(K) + 1e-5) * float(np.abs(ref).max())


# ---- plans: the enumeration of test_every_gemm_dispatch_choice_vs_fp64 ---------------------------------------------------------------------------
SKINNY = [(SMALLM, mt, kw, nt, 1) for nt in (1, 2, 4) for mt in (1, 2, 4) for kw in (4, 8, 16) if not ((mt >= 2 or nt == 4) and kw == 16)]
SKINNY_Z = [(SMALLM, mt, kw, nt, z) for (_, mt, kw, nt, _) in SKINNY for z in (2, 4, 8)]
TILED_PLANS = [(TILED, v, 0, 0, 1) for v in range(8)]
RING_PLANS = [(RING, v, 0, 0, 1) for v in range(7)]
SPLIT_PLANS = [(SPLIT, v, 0, 0, 1) for v in range(5)]
STREAM_PLANS = [(STREAM, mt, kw, nt, 1) for nt in (1, 2) for mt in (1, 2, 4) for kw in (4, 8, 16) if not (mt * nt > 2 and kw == 16)]
ALL_PLANS = SKINNY + TILED_PLANS + RING_PLANS + SPLIT_PLANS + STREAM_PLANS


def plan_name(p):
    return "%s %d,%d,%d,z%d" % (FAMILY_NAME[p[0]], p[1], p[2], p[3], p[4])


# ---- the plan check, restated (csrc/gemm_dispatch.hip plan_accepts + launch_conv_gemm_group_plan; gemm_pipe / gemm_split / gemm_stream *_supported) ----
def c_rows_vectorised(P):
    return (P["N"] % 4 == 0 and P["ldc"] % 4 == 0 and P["c_off"] % 4 == 0 and P["c_bstride"] % 4 == 0 and
            (not P["res"] or (P["ldr"] % 4 == 0 and P["r_off"] % 4 == 0 and P["r_bstride"] % 4 == 0)))


def a_aligned(P):
    return P["lda"] % 4 == 0 and P["a_off"] % 4 == 0 and P["a_bstride"] % 4 == 0


def pipe_gemm_supported(P):
    return (P["Cin"] % 64 == 0 and not P["dw"] and c_rows_vectorised(P) and a_aligned(P) and
            (not P["rms"] or (P["taps"] == 1 and P["Cin"] <= 2048 and not P["a_silu"])) and (not P["w13"] or P["N"] % 32 == 0))


def split_gemm_supported(P):
    return P["Cin"] % 32 == 0 and P["stride"] >= 1 and not P["rms"] and not P["dw"]


def stream_gemm_supported(P):
    return (P["Cin"] % 16 == 0 and a_aligned(P) and not P["dw"] and (not P["w13"] or P["N"] % 32 == 0) and
            (not P["rms"] or (P["taps"] == 1 and not P["a_silu"])))


def plan_accepts(plan, P, n=1):
    """P: the problem (of the lead member) as a dict -- M, T, N, Cin, taps, stride, the strides and offsets, res / rms / dw / w13 / a_silu flags"""
    fam, a, b, c, z = plan
    if P.get("planes"):
        return False                        # operands that exist only as planes (A / C null) are the planes kernel's: no fp32 family reads them
    if not (P["Cin"] > 0 and P["Cin"] % 16 == 0 and a_aligned(P) and (not P["w13"] or P["N"] % 32 == 0)):
        return False
    if n > 1 and (P["rms"] or P["dw"]):
        return False                        # conv_gemm_group_of
    cv = c_rows_vectorised(P)
    N = P["N"]
    if fam == SMALLM:
        if P["w13"] and c == 1:
            return False
        if P["rms"] and (P["taps"] != 1 or P["a_silu"] or n > 1):
            return False
        if P["dw"] and not (a == 1 and c == 1 and P["taps"] == 1 and P["stride"] == 1 and P["M"] <= 16 and P["Cin"] <= 512 and not P["a_silu"] and
                            not P["rms"] and not P["w13"] and n == 1):
            return False
        return (1 <= a <= 4 and (b in (4, 8) or (b == 16 and a == 1)) and
                (c == 1 or (c == 2 and N % 32 == 0) or (c == 4 and N % 64 == 0 and a != 3 and b != 16)) and 1 <= z <= 8 and (n == 1 or z == 1))
    if fam == TILED:
        return 0 <= a <= 7 and cv and not P["rms"] and not P["dw"] and not (P["w13"] and a == 3)
    if fam == RING:
        return 0 <= a <= 6 and cv and pipe_gemm_supported(P)
    if fam == SPLIT:
        return 0 <= a <= 4 and cv and split_gemm_supported(P)
    if fam == STREAM:
        tiles = (P["M"] + 16 * a - 1) // (16 * a) * ((N + 16 * c - 1) // (16 * c)) if a > 0 and c > 0 else 0
        return (n == 1 and stream_gemm_supported(P) and a in (1, 2, 4) and c in (1, 2) and (b in (4, 8) or (b == 16 and a * c <= 2)) and
                not (P["w13"] and c != 2) and tiles < 65536)
    raise ValueError(plan)


# (family, form) pairs no plan of the family takes, by design -- the reason is the kernel's, stated once:
#   the tiled and split kernels have no RMSNorm / ConvNeXt prologue; the ring kernel has the RMSNorm one (taps == 1) but no ConvNeXt one; the
#   weight-streaming kernel has no ConvNeXt prologue; the tiled, ring and split epilogues store 16-byte pieces of C rows, so a C whose rows are
#   not 16-byte aligned (E9) is for the small-M and weight-streaming kernels only.  (Plan-level refusals -- SwiGLU on one column tile per wave /
#   workgroup, the ConvNeXt prologue on anything but one 16 x 16 tile, two column tiles on N % 32 != 0 -- are plan_accepts' and are checked
#   plan by plan.)
REFUSED_BY_DESIGN = {
    (TILED, "E7"), (TILED, "E8"), (SPLIT, "E7"), (SPLIT, "E8"), (RING, "E8"), (STREAM, "E8"),
    (TILED, "E9"), (RING, "E9"), (SPLIT, "E9"),
}
FORM_SHAPE = {"E7": "P0t1", "E8": "PD"}          # the forms that need a shape of their own; every other form is checked on P0


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------
class Member:
    """one conv-GEMM problem on the host: geometry, operands as whole arrays with their padding, the index maps of C and of the residual"""

    def __init__(self, rng, shape, form, taps=None, dil=None, dense=False):
        s = dict(SHAPES[shape]) if isinstance(shape, str) else dict(shape)
        f = dict(FORMS, **FORMS_MORE)[form] if isinstance(form, str) else form
        self.f = f
        self.B, self.T, self.Cin, self.stride = s["B"], s["T"], s["Cin"], s["stride"]
        self.taps, self.dil = taps or s["taps"], dil or s["dil"]
        self.N = f.get("N", s["N"])
        self.w13 = bool(f.get("w13"))
        self.Nout = self.N // 2 if self.w13 else self.N
        self.M, self.K = self.B * self.T, self.taps * self.Cin
        self.dw = bool(f.get("dw"))
        B, T, Cin, N, K = self.B, self.T, self.Cin, self.N, self.K
        # A: two pad rows in front of everything, three pad rows behind every item's used rows, lda - Cin pad columns
        self.lda = Cin if dense else s["lda"]
        self.used = (T - 1) * self.stride + (self.taps - 1) * self.dil + 1 + (6 if self.dw else 0)
        self.a_off, self.a_bstride = 2 * self.lda, (self.used + 3) * self.lda
        A = np.where(np.arange(self.a_off + B * self.a_bstride) % 2 == 0, PAD, -PAD).astype(F32)
        x = rng.standard_normal((B, self.used, Cin)) + 0.05 * (np.arange(self.used) % 7)[None, :, None] + 0.02 * np.arange(Cin) / Cin
        W = (rng.standard_normal((N, K)) + 0.1 * (np.arange(N) % 5)[:, None] + 0.05 * np.arange(K) / K) / np.sqrt(K)
        if f.get("nonneg"):
            # log-clamp: non-negative operands, every tap row of two output rows all zero (the clamp branch), every other sum >= 2
            x, W = np.abs(x) + 0.25, np.abs(W) + 0.5 / np.sqrt(K)
            for (b, t) in ((0, 5), (B - 1, T - 1)):
                x[b, t * self.stride + np.arange(self.taps) * self.dil] = 0.0
        ai = (np.arange(B)[:, None, None] * self.a_bstride + self.a_off + np.arange(self.used)[None, :, None] * self.lda + np.arange(Cin)[None, None, :])
        A[ai] = x
        self.A, self.W = A, np.ascontiguousarray(W, F32)
        # C: c_off elements in front, pad columns Nout .. ldc, a tail between the items
        mis = "ldc" in f
        self.ldc = f.get("ldc", s["ldc"] - s["N"] + self.Nout if not dense else self.Nout)
        self.c_off = f.get("c_off", s["c_off"] if not dense else self.ldc)
        self.c_bstride = T * self.ldc + (3 if mis else (self.ldc if dense else 8))
        self.c_len = self.c_off + B * self.c_bstride
        self.cidx = (np.arange(B)[:, None, None] * self.c_bstride + self.c_off + np.arange(T)[None, :, None] * self.ldc + np.arange(self.Nout)[None, None, :])
        self.accumulate = bool(f.get("accumulate"))
        self.C0 = (rng.standard_normal(self.c_len) if self.accumulate else np.full(self.c_len, SENT)).astype(F32)
        self.bias = rng.standard_normal(N).astype(F32) if f.get("bias") else None
        self.gamma = rng.uniform(0.5, 1.5, N).astype(F32) if f.get("gamma") else None
        self.res = None
        self.ldr = self.r_off = self.r_bstride = 0
        if f.get("res"):                     # its own geometry: ldr != ldc, r_off != c_off
            self.ldr, self.r_off = self.ldc + 4, self.c_off + 8
            self.r_bstride = T * self.ldr + 4
            self.res = rng.standard_normal(self.r_off + B * self.r_bstride).astype(F32)
            self.ridx = (np.arange(B)[:, None, None] * self.r_bstride + self.r_off + np.arange(T)[None, :, None] * self.ldr + np.arange(self.Nout)[None, None, :])
        self.rms_w = rng.uniform(0.5, 1.5, Cin).astype(F32) if f.get("rms") else None
        self.dwp = None
        if self.dw:
            self.dwp = ((rng.standard_normal((7, Cin)) * 0.4).astype(F32), rng.standard_normal(Cin).astype(F32), rng.uniform(0.5, 1.5, Cin).astype(F32),
                        rng.standard_normal(Cin).astype(F32), 1e-6)
        self.act, self.scale, self.a_silu = f.get("act", 0), f.get("scale", 1.0), bool(f.get("a_silu"))
        self.skip = f.get("skip", (0, 0))
        self._ref = {}

    def problem(self):
        """the fields plan_accepts reads"""
        return dict(M=self.M, T=self.T, N=self.N, Cin=self.Cin, taps=self.taps, stride=self.stride, lda=self.lda, a_off=self.a_off, a_bstride=self.a_bstride,
                    ldc=self.ldc, c_off=self.c_off, c_bstride=self.c_bstride, res=self.res is not None, ldr=self.ldr, r_off=self.r_off, r_bstride=self.r_bstride,
                    w13=self.w13, a_silu=self.a_silu, rms=self.rms_w is not None, dw=self.dw)

    def plan_desc(self, operands=0, pmode=-1, cp_silu=False):
        """the 12 ints of sva_test_gemm_plan for this problem"""
        fl = ((1 if self.bias is not None else 0) | (2 if self.gamma is not None else 0) | (4 if self.res is not None else 0) | (8 if self.act == 1 else 0) |
              (16 if self.a_silu else 0) | (32 if self.w13 else 0) | (64 if self.accumulate else 0) | (128 if self.rms_w is not None else 0) |
              (256 if self.dw else 0) | (512 if cp_silu else 0))
        mis = (2 if not c_rows_vectorised(dict(self.problem(), res=False)) else 0)
        return [self.B, self.T, self.N, self.Cin, self.taps, self.stride, self.dil, fl, operands, pmode, mis, 0]

    def hook(self, **extra):
        """the member as engine.test_conv_gemm takes it, with a fresh copy of C"""
        m = dict(B=self.B, T=self.T, N=self.N, Cin=self.Cin, taps=self.taps, stride=self.stride, dil=self.dil, lda=self.lda, a_off=self.a_off,
                 a_bstride=self.a_bstride, A=self.A, W=self.W, bias=self.bias, gamma=self.gamma, res=self.res, ldr=self.ldr, r_off=self.r_off,
                 r_bstride=self.r_bstride, rms_w=self.rms_w, C=self.C0.copy(), ldc=self.ldc, c_off=self.c_off, c_bstride=self.c_bstride, act=self.act,
                 scale=self.scale, accumulate=int(self.accumulate), a_silu=int(self.a_silu), w13=int(self.w13), skip_lo=self.skip[0], skip_hi=self.skip[1])
        if self.dwp is not None:
            m.update(dw_wT=self.dwp[0], dw_b=self.dwp[1], ln_w=self.dwp[2], ln_b=self.dwp[3], ln_eps=self.dwp[4])
        m.update(extra)
        return m

    def rows(self, A=None):
        return R.conv_rows(self.A if A is None else A, self.B, self.T, self.Cin, taps=7 if self.dw else self.taps, stride=self.stride,
                           dil=1 if self.dw else self.dil, lda=self.lda, a_off=self.a_off, a_bstride=self.a_bstride)

    def ref(self, dt, rows=None, W=None, key=None):
        """[B, T, Nout] in precision dt (cached): the stored value of every (b, t, n), skipped rows included"""
        k = (dt, key)
        if k not in self._ref:
            rows = self.rows() if rows is None else rows
            self._ref[k] = R.conv_gemm(rows, self.W if W is None else W, bias=self.bias, act=self.act, gamma=self.gamma,
                                       res=None if self.res is None else self.res[self.ridx], scale=self.scale,
                                       c_in=self.C0[self.cidx] if self.accumulate else None, a_silu=self.a_silu, w13=self.w13, rms_w=self.rms_w,
                                       dw=self.dwp, dt=dt)
        return self._ref[k]

    def stored(self):
        """mask [B, T, Nout] of the elements a launch stores"""
        keep = np.ones((self.B, self.T, self.Nout), bool)
        keep[:, self.skip[0]:self.skip[1]] = False
        return keep

    def epilogue_gain(self, rows=None, W=None):
        """[B, T, Nout] (or a scalar): how much an error d of the raw product v moves the stored value, to first order with the function's largest
        slope -- |gamma| scale for the linear stages, 1.13 = max |gelu'| on top for GELU, 1 / v for the log of an un-clamped v (0 where clamped:
        the clamp absorbs it), and for SwiGLU silu(g) u: 1.1 |u| + |silu(g)| (max |silu'| = 1.1)"""
        rows = self.rows().astype(F64) if rows is None else rows
        W = self.W.astype(F64) if W is None else W
        a = R.silu(rows) if self.a_silu else rows
        v = a.reshape(self.B, self.T, -1) @ W.T
        if self.w13:
            g = v.reshape(self.B, self.T, self.N // 32, 2, 16)
            return (1.1 * np.abs(g[..., 1, :]) + np.abs(R.silu(g[..., 0, :]))).reshape(self.B, self.T, self.Nout)
        gain = np.ones_like(v)
        if self.bias is not None:
            v = v + self.bias
        if self.act == 1:
            gain *= 1.13
        elif self.act == 2:
            gain = np.where(v > float(R.LOG_CLAMP), 1.0 / np.maximum(v, float(R.LOG_CLAMP)), 0.0)
        if self.gamma is not None:
            gain = gain * np.abs(self.gamma)
        return gain * abs(self.scale)

    def split_extra(self):
        """gemm_split.hip computes six of the nine bf16 part products of x = hi + mid + lo (exact: 3 x 8 significand bits): the dropped ones,
        sum_k |a_mid w_lo| + |a_lo w_mid| + |a_lo w_lo|, through the epilogue's gain; the split itself is exact (asserted)"""
        if "split" not in self._ref:
            a = self.rows()
            if self.a_silu:
                a = R.silu(a, F32)
            a = np.ascontiguousarray(a.reshape(self.M, self.K), F32)
            ah, am, al = R.bf16_split3(a)
            wh, wm, wl = R.bf16_split3(self.W)
            assert np.array_equal(ah.astype(F64) + am + al, a.astype(F64)) and np.array_equal(wh.astype(F64) + wm + wl, self.W.astype(F64))
            am, al, wm, wl = (np.abs(p).astype(F64) for p in (am, al, wm, wl))
            d = (am @ wl.T + al @ wm.T + al @ wl.T).reshape(self.B, self.T, self.N)
            if self.w13:
                g = d.reshape(self.B, self.T, self.N // 32, 2, 16)
                v = (R.silu(self.rows().astype(F64)) if self.a_silu else self.rows().astype(F64)).reshape(self.B, self.T, -1) @ self.W.astype(F64).T
                vg = v.reshape(self.B, self.T, self.N // 32, 2, 16)
                e = 1.1 * np.abs(vg[..., 1, :]) * g[..., 0, :] + np.abs(R.silu(vg[..., 0, :])) * g[..., 1, :]
                self._ref["split"] = float(e.max())
            else:
                self._ref["split"] = float((d * self.epilogue_gain()).max())
        return self._ref["split"]


_CASES = {}


def case(shape, form, taps=None, dil=None, seed=0, dense=False):
    """the cached member of (shape, form): operands and references are computed once and shared by every plan"""
    key = (shape, form, taps, dil, seed, dense)
    if key not in _CASES:
        _CASES[key] = Member(np.random.default_rng(1000 + 7919 * seed + sum(ord(ch) for ch in shape + form) + 31 * (taps or 0)), shape, form, taps, dil, dense)
    return _CASES[key]


def shape_of(form):
    return FORM_SHAPE.get(form, "P0")
