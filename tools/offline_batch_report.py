"""What converting many offline utterances in one batch buys, measured on the GPU (InferenceWrapper.infer_many / sva_generate_many):

  (a) throughput: utterances/s and x real time of infer_many at n_slots 1 / 8 / 64 against the same utterances through sequential
      InferenceWrapper.infer calls (one-stream batch: encode_content + Batch.generate + vocode_window, the path that existed before), on
      SURVEY 8d config 3's synthetic material: 64 utterances of 10 s (215 frames), prompts of 5 s (107 frames); every arm runs the whole
      list `--repeats` times after one unmeasured pass (first launches of its shapes), wall clock around calls that end synchronised;
      the same on a ragged list (2 - 10 s, seeded) where finished slots ride along parked;
  (b) prefill cost: sva_generate_many with the shortest legal source (delay + 1 frames) and with 10 frames more -- their difference gives
      the cost of a decode frame, the rest is the prefill part with its packed runs passes -- against n sva_prefill_prompt calls (one
      ar_prefill_slot pass per slot) over prompts of the same row count, at n = 8 and 64;
  (c) parked frames: the share of decode frames (slots x frames of every wave) spent on slots that had already finished;
  (d) where a wave's time goes: the steps of infer_many for one wave of n 10 s utterances timed apart (batch creation, encode_window,
      generate_many, vocode_window, batch teardown), at n = 1 / 8 / 64.

    python tools/offline_batch_report.py [--out profiles/offline_batch_report.txt] [--utterances 64] [--repeats 2] [--slots 1 8 64] [--parts a b c d]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 2048
SR = 44100


def parked_share(lengths, waves):
    total = sum(len(w) * max(lengths[i] for i in w) for w in waves)
    return (total - sum(lengths)) / total


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offline_batch_report.txt"))
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--frames", type=int, default=215)
    ap.add_argument("--prompt-frames", type=int, default=107)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic waveforms (the list cycles through them; prompts and seeds differ)")
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c", "d"])
    args = ap.parse_args(argv)

    import torch
    from oracle import sva_oracle as O
    from streamvoiceanon_amd import engine as E, specs
    from streamvoiceanon_amd.infer_arvc import InferenceWrapper
    from streamvoiceanon_amd.stream_pool import plan_offline_waves
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

    if not torch.cuda.is_available():
        raise SystemExit("offline_batch_report: needs the GPU (nothing here is measured on a CPU)")
    torch.set_grad_enabled(False)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W = O.load_synth_weights(0, specs.all_specs())
    w = InferenceWrapper(weights=W)
    n_utt, F, R, d = args.utterances, args.frames, args.prompt_frames, 2
    base = [synth_utterance(1000 + u, N * F) for u in range(min(args.distinct, n_utt))]
    prompts = [synth_prompt(2000 + u, R) for u in range(n_utt)]
    seeds = [1000 + u for u in range(n_utt)]
    rng = np.random.default_rng(64)
    lists = {"10 s": [F] * n_utt, "ragged 2 - 10 s": [int(x) for x in rng.integers(F // 5, F + 1, n_utt)]}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    say("offline batches: InferenceWrapper.infer_many against sequential InferenceWrapper.infer (one-stream batch), %s" % torch.cuda.get_device_name(0))
    say("%d utterances, prompts of %d frames, delay %d, fp32 AR, device RNG; wall clock, median [min - max] of %d passes over the list after one "
        "unmeasured pass" % (n_utt, R, d, args.repeats))
    say()
    say("(a) throughput")
    say("%-18s %-22s %28s %14s %12s %10s" % ("list", "arm", "wall s", "utterances/s", "x real time", "vs infer"))
    ratios = {}
    for name, lens in lists.items() if "a" in args.parts else ():
        srcs = [base[u % len(base)][:N * lens[u]] for u in range(n_utt)]
        audio_s = sum(lens) * N / SR
        arms = [("sequential infer", lambda: [w.infer(s, prompt=p, delay=d, save_result=False, noise_seed=sd) for s, p, sd in zip(srcs, prompts, seeds)])]
        for ns in args.slots:
            arms.append(("infer_many n_slots=%d" % ns, lambda ns=ns: w.infer_many(srcs, prompts=prompts, n_slots=ns, delay=d, noise_seeds=seeds)))
        ref = None
        for arm, fn in arms:
            try:
                fn()                                      # unmeasured: first launches of this arm's shapes
                t = [timed(fn) for _ in range(args.repeats)]
            except RuntimeError as err:                   # (a wave's batch that cannot be allocated: reported, not hidden)
                say("%-18s %-22s failed: %s" % (name, arm, str(err)[:200]))
                continue
            med = statistics.median(t)
            ref = med if ref is None else ref
            ratios[(name, arm)] = ref / med
            say("%-18s %-22s %28s %14.2f %12.1f %10.2f" % (name, arm, "%.3f [%.3f - %.3f]" % (med, min(t), max(t)), n_utt / med, audio_s / med, ref / med))
    say()
    say("(b) prefill part of sva_generate_many (packed runs passes) against n sva_prefill_prompt calls (one pass per slot); prompts of %d + %d frames "
        "= %d rows each; ms, wall, median of %d" % (R, d, 33 + 2 * (R + d) + 1, max(3, args.repeats)))
    say("%6s %16s %16s %14s %18s %22s %8s" % ("n", "many, S = %d" % (d + 1), "many, S = %d" % (d + 11), "per frame", "many: prefill part", "n x prefill_prompt", "ratio"))
    for n in (8, 64) if "b" in args.parts else ():
        b = E.Batch(w.engine, n_streams=n, delay=d)
        try:
            pr = [(p[1], p[0], p[2], p[3]) for p in prompts[:n]]
            codes = lambda S: [(np.arange(S, dtype=np.int64) * 2654435761 % 8192).astype(np.int64) for _ in range(n)]
            ext = [(np.concatenate([p[1], codes(d)[0]]), np.concatenate([p[0], np.zeros((8, d), p[0].dtype)], 1), p[2], p[3]) for p in prompts[:n]]
            reps = max(3, args.repeats)

            def many(S):
                b.generate_many(pr, codes(S), noise_seeds=seeds[:n])

            def per_slot():
                for s in range(n):
                    b.prefill_prompt(s, ext[s][0], ext[s][1], ext[s][2], ext[s][3], noise_seed=seeds[s])

            many(d + 1); many(d + 11); per_slot()
            t3 = statistics.median([timed(lambda: many(d + 1)) for _ in range(reps)]) * 1e3
            t13 = statistics.median([timed(lambda: many(d + 11)) for _ in range(reps)]) * 1e3
            tp = statistics.median([timed(per_slot) for _ in range(reps)]) * 1e3
            frame = (t13 - t3) / 10
            pre = t3 - (d + 1) * frame
            say("%6d %16.2f %16.2f %14.3f %18.2f %22.2f %8.2f" % (n, t3, t13, frame, pre, tp, tp / pre))
        finally:
            b.close()
    say()
    say("(c) parked frames: share of the decode frames of all waves (slots x frames) spent on slots that had finished")
    for name, lens in lists.items():
        say("%-18s %s" % (name, "   ".join("n_slots=%d: %.1f %%" % (ns, 100 * parked_share(lens, plan_offline_waves(lens, ns))) for ns in args.slots)))
    say()
    say("(d) waves of n utterances of %d frames through the steps of infer_many, timed apart, a fresh batch per wave; ms, wall, each step ends "
        "synchronised; median (max) over the waves after one unmeasured wave" % F)
    say("%6s %6s %18s %18s %18s %18s %18s %14s" % ("n", "waves", "Batch()", "encode_window", "generate_many", "vocode_window", "close()", "per utterance"))
    for n in args.slots if "d" in args.parts else ():
        Wp = ((F + 3) // 4) * 4
        buf = np.zeros((n, Wp * N), np.float32)
        for k in range(n):
            buf[k, :F * N] = base[k % len(base)][:F * N]
        pr = [(p[1], p[0], p[2], p[3]) for p in prompts[:n]]
        n_waves = max(1, min(8, n_utt // n))
        rows = []
        for rep in range(n_waves + 1):
            t, st = [], {}
            t.append(timed(lambda: st.update(b=E.Batch(w.engine, n_streams=n, encode_window_frames=Wp, voc_max_frames=F, delay=d))))
            b = st["b"]
            try:
                t.append(timed(lambda: st.update(cc=b.encode_window(buf))))
                t.append(timed(lambda: st.update(codes=b.generate_many(pr, [st["cc"][k, :F] for k in range(n)], noise_seeds=seeds[:n]))))
                t.append(timed(lambda: b.vocode_window(np.stack(st["codes"]))))
            finally:
                t.append(timed(b.close))
            if rep:
                rows.append([x * 1e3 for x in t])
        cols = list(zip(*rows))
        say("%6d %6d %s %14.1f" % (n, n_waves, " ".join("%18s" % ("%.1f (%.1f)" % (statistics.median(c), max(c))) for c in cols),
                                   sum(statistics.median(c) for c in cols) / n))
    w.close()
    w.engine.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return ratios


if __name__ == "__main__":
    main()
