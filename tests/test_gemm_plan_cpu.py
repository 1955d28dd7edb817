"""The conv-GEMM dispatcher's decisions, pinned without a GPU (csrc/gemm_dispatch.hip: plan_conv_gemm through sva_test_gemm_plan).

Every case below is planned and compared, exactly, with tests/golden/gemm_plan_pin.npz: what the dispatcher decided for the same case list
BEFORE the decision became a function of its own (recorded from that commit's launch_conv_gemm_impl, patched to return its choice instead of
launching).  The fixture holds the old encoding {Choice.kind, a, b, c, z, last_kind}; PARENT_KIND maps a family onto it."""
import os
import re
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "streamvoiceanon_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plan_pin.npz")

# descriptor bits of sva_test_gemm_plan (include/sva.h)
BIAS, GAMMA, RES, GELU, A_SILU, W13, ACC, RMS, DWLN, CP_SILU = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
WK, WH, WKH, WP, AP, CP = 1, 2, 4, 8, 16, 32
H3, H1 = 1, 2
SMALL_M, TILED, RING, SPLIT, F16W, STREAM, PLANES, PLANES_DMA, STREAM_H = range(9)
# family -> (Choice.kind, offset of Choice.a) of the dispatcher before the refactor: the planes kernel was "split kernel, variant + 8"; the
# fp16-weight and fp16-operand kernels had no Choice (recorded as kind 5 / 11 with zero parameters)
PARENT_KIND = {SMALL_M: (0, 0), TILED: (1, 0), RING: (2, 0), SPLIT: (4, 0), F16W: (5, 0), STREAM: (6, 0), PLANES: (4, 8), PLANES_DMA: (4, 8), STREAM_H: (11, 0)}
AR_SHAPES = [(768, 768, 0), (2304, 768, 0), (4608, 768, W13), (768, 2304, 0)]         # (N, K, flags)


def mem(M, N, Cin, taps=1, stride=1, dil=1, flags=0, ops=0, pmode=-1, mis=0, B=1):
    assert M % B == 0
    return (B, M // B, N, Cin, taps, stride, dil, flags, ops, pmode, mis, 0)


def tune_rows():
    rows = []
    for line in open(os.path.join(CSRC, "tune_table.inc")):
        m = re.match(r"\s*\{\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}, (\d+), (\d+), (\d+), (\d+), (\d+)\}", line)
        if m:
            rows.append(tuple(int(x) for x in m.groups()))
    return rows


def planes_rows():
    rows = []
    for line in open(os.path.join(CSRC, "planes_table.inc")):
        m = re.match(r"\s*\{(\d+), (\d+), (\d+), (\d+)\}", line)
        if m:
            rows.append(tuple(int(x) for x in m.groups()))
    return rows


def row_members(row, ops=0, pmode=-1):
    """the problem (or group of three) a tune_table.inc key stands for"""
    M, N, K, taps, kf, stride = row[:6]
    flags = (A_SILU if kf & 1 else 0) | (RMS if kf & 2 else 0) | (W13 if kf & 4 else 0) | (ACC if kf & 16 else 0) | (DWLN if kf & 64 else 0)
    mis = 0 if kf & 8 else 2
    if not kf & 32:
        return [mem(M, N, K // taps, taps, stride, flags=flags, ops=ops, pmode=pmode, mis=mis)]
    return [mem(M, N, K // taps, t, stride, flags=flags, ops=ops, pmode=pmode, mis=mis) for t in (min(3, taps), min(7, taps), taps)]


def cases():
    """[(section, debug options, members)], deterministic"""
    out = []
    add = lambda sec, members, cfg="": out.append((sec, cfg, list(members)))
    # A: every row of the tuned table, with plain weights and with weight planes in H3 / H1
    for row in tune_rows():
        add("table", row_members(row))
        add("table", row_members(row, WP, H3))
        add("table", row_members(row, WP, H1))
    # B: row borrowing over the AR decode shapes
    for N, K, fl in AR_SHAPES:
        for M in range(8, 521, 4):
            add("borrow", [mem(M, N, K, flags=fl)])
            add("borrow", [mem(M, N, K, flags=fl | RMS)])
    # C: the heuristic, off the table
    for M in (1, 16, 48, 64, 65, 200, 512, 1000, 2048, 3072, 8192, 16384):
        for N in (16, 32, 48, 64, 96, 128, 512, 1000, 3072):
            for Cin in (64, 128, 512, 1536):
                for taps in (1, 7):
                    add("heuristic", [mem(M, N, Cin, taps)])
                    add("heuristic", [mem(M, N, Cin, taps, mis=2)])
    # D: operands as planes -- the encoder's GEMMs at the (N, K) pairs of planes_table.inc, the HiFiGAN levels' grouped convs
    prow = planes_rows()
    for cfg in ("", "planes_dma=0", "planes_lw=0"):
        for N, K in sorted({(r[1], r[2]) for r in prow}):
            tab_m = sorted(r[0] for r in prow if (r[1], r[2]) == (N, K))
            per_stream = tab_m[0] // 24 if tab_m[0] % 24 == 0 else 85          # (the tables start at 24 streams)
            by_streams = sorted(per_stream * s for s in (10, 12, 24, 48, 64, 128))
            near_table = sorted({int(m * f) for m in (tab_m[0], tab_m[-1]) for f in (0.7, 1.3)})
            for M in by_streams + near_table:
                for pm in (H3, H1):
                    add("planes", [mem(M, N, K, flags=BIAS, ops=WP | AP | CP, pmode=pm)], cfg)
            if not cfg:
                for M in by_streams:
                    add("planes", [mem(M, N, K, flags=BIAS | GELU, ops=WP | AP, pmode=H3)], cfg)
                    add("planes", [mem(M, N, K, flags=GAMMA | RES, ops=WP | CP, pmode=H3)], cfg)
        for N in (64, 128, 256, 512):
            for B, T in ((10, 160), (64, 160), (64, 640), (12, 2560)):
                for pm in (H3, H1):
                    for fl in (BIAS, BIAS | CP_SILU, BIAS | RES):
                        conv = lambda t, dil: mem(B * T, N, N, t, dil=dil, flags=fl, ops=WP | AP | (CP if fl & CP_SILU else 0), pmode=pm, B=B)
                        for t in (3, 7, 11):
                            add("planes_conv", [conv(t, 1)], cfg)
                        add("planes_conv", [conv(3, 1), conv(7, 3), conv(11, 5)], cfg)
    # E: fp16 weights (ar_dtype = 1), fp16 operands (enc_dtype = 1)
    for M in (1, 64, 256, 257, 1024):
        for N, K, fl in AR_SHAPES:
            add("f16w", [mem(M, N, K, flags=fl, ops=WH)])
            add("f16w", [mem(M, N, K, flags=fl | RMS, ops=WH)])
            add("f16w", [mem(M, N, K, flags=fl | (0 if fl else RES), ops=WH | WK)])
    for M in (16, 1023, 1024, 8192):
        for N, K in ((512, 512), (1536, 512), (128, 512), (2048, 512), (512, 2048), (32, 64), (16, 64)):
            for fl in (BIAS, BIAS | GELU, GAMMA | RES):
                add("wkh", [mem(M, N, K, flags=fl, ops=WKH)])
                add("wkh", [mem(M, N, K, flags=fl, ops=WKH | WP, pmode=H1)])
                add("wkh", [mem(M, N, K, flags=fl, ops=WKH | WP, pmode=H3)])
                add("wkh", [mem(M, N, K, flags=fl, ops=WKH | WP | AP | CP, pmode=H1)])
                add("wkh", [mem(M, N, K, flags=fl, ops=WKH | WP | AP, pmode=H1)], "planes_dma=0")
        add("wkh", [mem(M, 1024, 512, flags=W13, ops=WKH | WP, pmode=H1)])
        add("wkh", [mem(M, 512, 128, 7, flags=BIAS, ops=WKH | WP, pmode=H1)])
    # the fused ConvNeXt prologue, strided convs, misaligned residual, grouped launches off the table
    for M in (1, 8, 16):
        add("misc", [mem(M, 512, 128, flags=DWLN | BIAS | GELU)])
        add("misc", [mem(M, 1536, 384, flags=DWLN | BIAS | GELU, ops=WK)])
    for M in (64, 1000, 4096):
        add("misc", [mem(M, 256, 128, 4, stride=2)])
        add("misc", [mem(M, 256, 128, flags=RES, mis=4)])
        add("misc", [mem(M, 128, 128, t, flags=A_SILU | BIAS, ops=WK) for t in (3, 7, 11)])
        add("misc", [mem(M, 128, 128, t, flags=A_SILU | BIAS | ACC, ops=WP, pmode=H3) for t in (3, 7, 11)])
    return out


# refusals of the entry path: (members, message of the check that refuses)
REFUSALS = [
    ([mem(64, 128, 24)], "conv_gemm: Cin must be a multiple of 16"),
    ([mem(64, 128, 64, mis=1)], "conv_gemm: A must be float4-aligned"),
    ([mem(64, 48, 64, flags=W13)], "conv_gemm: w13 needs N % 32 == 0"),
    ([mem(2048, 3072, 768, flags=RMS)], "conv_gemm: fused RMSNorm needs taps == 1 on the small-M path"),
    ([mem(16, 768, 768, 3, flags=RMS)], "conv_gemm: fused RMSNorm needs taps == 1 on the small-M path"),
    ([mem(32, 512, 128, flags=DWLN)], "conv_gemm: the fused ConvNeXt prologue needs taps == 1, M <= 16, Cin <= 512"),
    ([mem(4096, 512, 512, ops=AP | CP)], "conv_gemm: operand planes handed to a problem the planes kernel does not take"),
    ([mem(4096, 512, 528, ops=WP | AP, pmode=H3)], "conv_gemm: operand planes handed to a problem the planes kernel does not take"),
    ([mem(4096, 512, 512, ops=WKH | AP)], "conv_gemm: operand planes handed to a problem the planes kernel does not take"),
    ([mem(64, 512, 512, flags=A_SILU, ops=WKH)], "conv_gemm: an fp16-operand layer that neither the planes kernel nor the fp16 weight-streaming kernel takes"),
    ([mem(64, 512, 512, ops=WKH)] * 2, "conv_gemm: fp16-operand layers take single problems"),
    ([mem(64, 128, 128, 3), mem(64, 256, 128, 7)], "conv_gemm_group: members must share shape and epilogue"),
    ([mem(64, 128, 128, 3), mem(64, 128, 128, 7, mis=1)], "conv_gemm_group: alignment classes must match"),
    ([mem(0, 128, 128)], "conv_gemm: empty problem"),
]


def case_digest(cs):
    return zlib.crc32(repr(cs).encode())


def run_cases(plan_fn, configure):
    """[rc, 6 numbers] per case through plan_fn(members) -> 6-tuple, raising RuntimeError on a refusal"""
    cs = cases()
    res = np.zeros((len(cs), 7), np.int32)
    cfg_now = ""
    try:
        for i, (_, cfg, members) in enumerate(cs):
            if cfg != cfg_now:
                configure(b"planes_dma=1,planes_lw=1")
                if cfg:
                    configure(cfg.encode())
                cfg_now = cfg
            try:
                res[i, 1:] = plan_fn(members)
            except RuntimeError:
                res[i, 0] = -1
    finally:
        configure(b"planes_dma=1,planes_lw=1")
    return cs, res


@pytest.fixture(scope="module")
def planned():
    from streamvoiceanon_amd import engine as E

    assert "SVA_DEBUG" not in os.environ, "the pinned decisions are the default ones"
    cs, res = run_cases(E.test_gemm_plan, E.load_library().sva_debug_configure)
    fx = np.load(FIXTURE)
    assert int(fx["digest"]) == case_digest(cs) and len(fx["plans"]) == len(cs), "the case list changed: the fixture no longer describes it"
    return cs, res, fx["plans"].astype(np.int32)


def as_parent(res):
    """the new plans in the fixture's encoding"""
    out = res.copy()
    for i in np.nonzero(res[:, 0] == 0)[0]:
        kind, off = PARENT_KIND[int(res[i, 1])]
        out[i, 1], out[i, 2] = kind, res[i, 2] + off
    return out


def test_every_plan_equals_the_pinned_decision(planned):
    cs, res, want = planned
    got = as_parent(res)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(cs[i], got[i].tolist(), want[i].tolist()) for i in bad[:10]]


def test_fixture_covers_every_family_and_report_kind(planned):
    cs, res, want = planned
    ok = res[res[:, 0] == 0]
    assert set(ok[:, 1].tolist()) == set(range(9)), sorted(set(ok[:, 1].tolist()))
    assert set(ok[:, 6].tolist()) == {0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11}, sorted(set(ok[:, 6].tolist()))
    assert set(want[want[:, 0] == 0][:, 6].tolist()) == {0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11}
    assert 2000 <= len(cs) <= 9000


def test_borrowed_rows_are_taken(planned):
    """an untabulated row count takes the row of the next larger tabulated one within 1.5 x"""
    cs, res, _ = planned
    table = {r[:6]: r[6:] for r in tune_rows()}
    family_of = {0: SMALL_M, 1: TILED, 2: RING, 4: SPLIT, 6: STREAM}
    taken = 0
    for (sec, _, members), r in zip(cs, res):
        if sec != "borrow" or r[0] != 0:
            continue
        B, T, N, Cin, taps, stride, _, fl = members[0][:8]
        M = B * T
        key = lambda m: (m, N, Cin * taps, taps, 8 | (2 if fl & RMS else 0) | (4 if fl & W13 else 0), stride)
        if key(M) in table:
            continue
        larger = [m for m in range(M + 1, M + M // 2 + 1) if key(m) in table]
        if larger:
            kind, a, b, c, z = table[key(larger[0])]
            taken += tuple(r[1:6]) == (family_of[kind], a, b, c, z)
    assert taken >= 10, taken


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_keep_their_message(i):
    from streamvoiceanon_amd import engine as E

    members, msg = REFUSALS[i]
    with pytest.raises(RuntimeError) as e:
        E.test_gemm_plan(members)
    assert str(e.value).split(": ", 1)[1].startswith(msg + " ["), str(e.value)


def test_every_table_row_passes_the_plan_validator(planned):
    """plan_accepts doubles as the table-row filter: every row of tune_table.inc, presented as the problem it was tuned on, is honoured"""
    cs, res, _ = planned
    family_of = {0: SMALL_M, 1: TILED, 2: RING, 4: SPLIT, 6: STREAM}
    rows = tune_rows()
    plain = [r for (sec, _, m), r in zip(cs, res) if sec == "table" and m[0][8] == 0]
    assert len(plain) == len(rows)
    for row, r in zip(rows, plain):
        assert r[0] == 0 and tuple(r[1:6]) == (family_of[row[6]],) + row[7:], (row, r.tolist())
