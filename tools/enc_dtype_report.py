"""What sva_config.enc_dtype = 1 (fp16-operand content encoder) costs and buys, measured on the GPU in one process:

  (i)   encoder stage time (sva_get_timings over eager, synchronised steps) for enc_dtype 0 and 1 at 1, 8 and 64 streams: median of 3
        repeats of 50 steps, the two modes' repeats alternating, with the spread (max - min of the repeats' medians);
  (ii)  per covered GEMM shape of the single-stream step: microseconds of the fp16 weight-streaming kernel (sva_test_gemm_h16, 200
        launches) beside the dispatcher's fp32 choice for the same shape and epilogue (sva_bench_gemm_choice, kind -1);
  (iii) agreement of the mode's content codes with the fp32 reference fixtures encoder_s0, encoder_s1 and the first 64 chunks of
        stream_long_reprefill.

    python tools/enc_dtype_report.py [--out profiles/enc_fp16_report.txt] [--streams 1 8 64]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_fp16_report.txt"))
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    torch.set_grad_enabled(False)
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import engine as E, specs
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance
    from enc_fp16_ref import agreement

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W = O.load_synth_weights(0, specs.all_specs(prompt_path=True))
    engines = {0: E.Engine(W, enc_dtype=0), 1: E.Engine(W, enc_dtype=1)}
    ac, cc, style, timbre = synth_prompt(2000, 107)

    def stream_batch(eng, B, profile=False):
        b = E.Batch(eng, n_streams=B)
        for s in range(B):
            b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=1000 + s)
        b.begin()
        return b

    # ---- (i) encoder stage -----------------------------------------------------------------------------------------------------------
    say("(i) encoder stage of the eager synchronised step, ms: median of %d repeats of %d steps (spread = max - min of the repeats' medians)" % (args.repeats, args.steps))
    say("%8s %22s %22s %10s %s" % ("streams", "enc_dtype=0", "enc_dtype=1", "1 / 0", "verdict"))
    headline = {}
    for B in args.streams:
        src = np.stack([synth_utterance(1000 + s, 2048 * 8) for s in range(min(B, 8))])
        src = np.concatenate([src] * ((B + 7) // 8))[:B]
        batches = {m: stream_batch(engines[m], B) for m in (0, 1)}
        k = {0: 0, 1: 0}

        def steps(m, n):
            out = []
            for _ in range(n):
                i = k[m] % 8
                k[m] += 1
                batches[m].step(src[:, i * 2048:(i + 1) * 2048])
                out.append(batches[m].timings()["encoder"])
            return out
        for m in (0, 1):
            steps(m, 10)
        meds = {0: [], 1: []}
        for _ in range(args.repeats):
            for m in (0, 1):
                meds[m].append(float(np.median(steps(m, args.steps))))
        for m in (0, 1):
            batches[m].close()
        med = {m: float(np.median(meds[m])) for m in (0, 1)}
        spr = {m: max(meds[m]) - min(meds[m]) for m in (0, 1)}
        gain = med[0] - med[1]
        verdict = "lower by more than the spread" if gain > max(spr.values()) else ("NOT lower by more than the spread" if gain > 0 else "NOT lower")
        headline[B] = (med[0], med[1])
        say("%8d %12.3f +- %6.3f %12.3f +- %6.3f %10.3f %s" % (B, med[0], spr[0], med[1], spr[1], med[1] / med[0], verdict))
    say()

    # ---- (ii) per GEMM shape of the single-stream step ---------------------------------------------------------------------------------
    b = stream_batch(engines[1], 1)
    x = synth_utterance(1000, 2048 * 4)
    for i in range(3):
        b.step(x[None, i * 2048:(i + 1) * 2048])
    b.profile_gemm(True)
    b.step(x[None, 3 * 2048:])
    b.sync()
    tab = b.gemm_profile_table()
    b.close()
    kind = (tab[:, 4].astype(np.int64) // 256) - 1
    shapes = {}
    for row, kd in zip(tab, kind):
        if kd != 11:
            continue
        key = (int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[4]) % 256)
        shapes[key] = shapes.get(key, 0) + 1
    say("(ii) covered GEMM shapes of the single-stream step (enc_dtype = 1: all on gemm_stream_h.hip), us per launch, 200 back-to-back launches on one")
    say("     weight copy; fp32 = the dispatcher's choice for the shape and epilogue WITHOUT the prologues it fuses at this size (dwconv7 + LayerNorm into")
    say("     pwconv1 up to 16 rows, RMSNorm into wqkv / w13), which enc_dtype = 1 runs as launches of their own: (i) is the whole account")
    say("%6s %6s %6s %5s %5s %6s %10s %10s %8s" % ("M", "N", "K", "taps", "epi", "count", "fp32 us", "fp16 us", "16 / 32"))
    rng = np.random.RandomState(0)
    slower = []
    tot32 = tot16 = 0.0
    for (M, N, K, taps, fl), cnt in sorted(shapes.items()):
        Cin, stride = K // taps, (2 if taps == 2 else 1)
        rows = (M - 1) * stride + (taps - 1) + 1
        A = rng.uniform(-1, 1, (1, rows, Cin)).astype(np.float32)
        Wm = (rng.uniform(-1, 1, (N, K)) * 0.05).astype(np.float32)
        swiglu, gelu, gres = bool(fl & 8), bool(fl & 1), bool(fl & 2)
        _, us16 = E.test_gemm_h16(A, Wm, 1, M, taps=taps, stride=stride, bias=None if swiglu else np.zeros(N, np.float32), gelu=gelu, swiglu=swiglu,
                                  gamma=np.ones(N, np.float32) if gres else None, res=np.zeros((1, M, N), np.float32) if gres else None, iters=200)
        us32 = E.bench_gemm_choice(1, M, N, Cin, -1, taps=taps, mode=fl & 11, nrot=1, iters=200)[0]
        tot32 += cnt * us32
        tot16 += cnt * us16
        if us16 > us32:
            slower.append((M, N, K, taps))
        say("%6d %6d %6d %5d %5d %6d %10.2f %10.2f %8.2f" % (M, N, K, taps, fl, cnt, us32, us16, us16 / us32))
    say("sum over the step's launches: fp32 %.1f us, fp16 %.1f us (%.2f)" % (tot32, tot16, tot16 / max(tot32, 1e-9)))
    say("shapes where the fp16 kernel is SLOWER than the fp32 choice: %s" % (slower if slower else "none"))
    say()

    # ---- (iii) agreement with the fp32 reference fixtures --------------------------------------------------------------------------------
    def golden(name):
        return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))

    say("(iii) content codes of enc_dtype = 1 against the fp32 reference fixtures: equal bits / equal whole codes, max |du| where the fixture has u")
    g = golden("encoder_s0")
    wb = E.Batch(engines[1], n_streams=1)
    codes, u = wb.encode_window(synth_utterance(int(g["audio_seed"]), int(g["n_samples"]))[None], return_u=True)
    wb.close()
    bits, whole = agreement(codes[0], g["codes"])
    say("encoder_s0             bits %.4f %%  codes %.2f %%  max|du| %.3g" % (100 * bits, 100 * whole, np.abs(u[0] - g["u"]).max()))
    agree = {"encoder_s0": (bits, whole)}
    g = golden("encoder_s1")
    W1 = dict(W)
    W1.update(O.load_synth_weights(1, specs.tokenizer_specs()))
    e1 = E.Engine(W1, enc_dtype=1)
    wb = E.Batch(e1, n_streams=1)
    codes, u = wb.encode_window(synth_utterance(int(g["audio_seed"]), int(g["n_samples"]))[None], return_u=True)
    wb.close()
    e1.close()
    bits, whole = agreement(codes[0], g["codes"])
    say("encoder_s1             bits %.4f %%  codes %.2f %%  max|du| %.3g" % (100 * bits, 100 * whole, np.abs(u[0] - g["u"]).max()))
    agree["encoder_s1"] = (bits, whole)
    g = golden("stream_long_reprefill")
    acp, ccp, stp, tmp = synth_prompt(int(g["prompt_seed"]), int(g["prompt_frames"]))
    b = E.Batch(engines[1], n_streams=1, chunk_frames=int(g["chunk"]), delay=int(g["delay"]), max_seq_frames=int(g["max_seq_frames"]),
                buffer_frames=int(g["buffer_frames"]))
    b.prefill_prompt(0, ccp, acp, stp, tmp, noise_seed=int(g["audio_seed"]))
    b.begin()
    src = synth_utterance(int(g["audio_seed"]), 2048 * int(g["n_chunks"]))
    got = []
    for i in range(64):
        b.step(src[None, i * 2048:(i + 1) * 2048])
        got.append(int(b.tap("content_codes", (1, 1), np.int32)[0, 0]))
    b.close()
    bits, whole = agreement(np.array(got), g["content_codes"][:64])
    say("stream_long_reprefill  bits %.4f %%  codes %.2f %%  (first 64 chunks, streaming step)" % (100 * bits, 100 * whole))
    agree["stream_long_reprefill"] = (bits, whole)
    say()
    say("headline: encoder stage enc_dtype 0 -> 1: " + ", ".join("%d streams %.2f -> %.2f ms" % (B, v[0], v[1]) for B, v in headline.items()) +
        "; code bits equal to the fp32 fixtures: " + ", ".join("%s %.2f %%" % (k, 100 * v[0]) for k, v in agree.items()))
    for e in engines.values():
        e.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
