"""What restarting single streams inside a running batch costs and buys, measured on the GPU:

  (a) wall time of sva_stream_restart and the stall of the step that activates the restarted slot (its wall time minus the median
      steady step of the same batch; synchronised host-buffer steps) at 2 / 8 / 64 streams with chunk 1, median of `--repeats` restarts;
  (b) frames/s of InferenceWrapper.stream_infer_many over a seeded list of 3 x n_slots utterances of 20-120 chunks at 8 and 64 slots,
      against the same list run as lock-step waves with the calls that existed before (one fresh batch per n_slots utterances, every
      slot running to the wave's longest utterance; frames counted are the utterances' own);
  (c) `python bench.py` and `python bench.py --streams 64`, `--bench-runs` runs each, in this tree and in a checkout of the parent
      commit (--parent-root DIR, built there), the runs of the two trees alternating;
  plus whether the restarted slot's PCM is bit-equal to its twin's (the question tests/test_gpu_stream_restart.py leaves open).

    python tools/stream_restart_report.py [--out profiles/stream_restart_report.txt] [--parent-root DIR] [--skip a b c]

--slot-priming: the A/B arm of slot-local activation (sva_stream_params.slot_priming).  Parts (a) and (b) are measured for slot_priming 0 and
1 in this one process, the two settings alternating per repeat (a fresh batch per repeat and setting, one unmeasured warm-up of each first);
every cell is median [min - max].  (a) adds the split of the stall from Batch.activations(): last_ms = prompt prefill + delay fill + vocoder
priming of the activation, the rest = draining the step and the step itself, and the device memory a batch takes with either setting (free memory around its
creation: what the priming workspace costs).  Default output: profiles/slot_priming_report.txt
(profiles/stream_restart_report.txt stays as the record of the whole-batch path alone).  --twin-pcm FILE appends the per-form twin-PCM
differences recorded by tests/test_gpu_slot_priming.py (a junit xml of that file's run).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK_MS = 2048 / 44100 * 1e3          # 46.4 ms of audio per chunk at chunk_frames = 1


def cell(v, fmt="%.2f"):
    return (fmt + " [" + fmt + " - " + fmt + "]") % (statistics.median(v), min(v), max(v))


def slot_priming_a(say, E, eng, prompt, synth_utterance, streams, repeats):
    """(a) for both settings -> {B: {setting: [stall per repeat]}}"""
    import torch

    ac, cc, style, timbre = prompt
    say("(a) the step that activates a restarted slot, chunk 1, delay 2, prompt 107 frames, slot_priming 0 | 1 alternating per repeat: "
        "median [min - max] of %d restarts (ms, wall, synchronised steps)" % repeats)
    say("%8s %3s %24s %26s %26s %26s %26s %10s %14s" % ("streams", "sp", "steady step", "activating step", "stall", "activation (last_ms)",
                                                         "stall - last_ms", "stall/chunk", "twin max |d|"))
    stalls = {}
    for B in streams:
        utt = synth_utterance(1000, 2048 * 12)
        src = np.repeat(utt[None], B, 0)
        res = {sp: dict(steady=[], act=[], stall=[], last=[], rest=[], diff=0.0, counts=None) for sp in (0, 1)}
        mem = {}
        for r in range(-1, repeats):                     # r = -1: warm-up of both settings (first launches of the T = P shapes), not recorded
            for sp in (0, 1):
                free0 = torch.cuda.mem_get_info(0)[0]
                b = E.Batch(eng, n_streams=B, slot_priming=bool(sp))
                if r < 0:
                    mem[sp] = (free0 - torch.cuda.mem_get_info(0)[0]) / 2**20      # device memory the batch took (whole arena chunks)
                for s in range(B):
                    b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=1000)
                b.begin()
                first = [b.step(src[:, k * 2048:(k + 1) * 2048])[0].copy() for k in range(12)]        # slot 0 from the batch's start: the twin
                slot = B - 1
                b.sync()
                b.restart(slot, cc, ac, style, timbre, noise_seed=1000)
                t_steady, t_act, diff = [], None, 0.0
                for k in range(12):
                    x = src[:, k * 2048:(k + 1) * 2048]
                    t0 = time.perf_counter()
                    y = b.step(x)
                    dt = (time.perf_counter() - t0) * 1e3
                    if k == 1:                           # delay 2: the slot activates at the end of its second step
                        t_act = dt
                    else:
                        t_steady.append(dt)
                    diff = max(diff, float(np.abs(y[slot] - first[k]).max()))
                n_local, n_whole, last_ms = b.activations()
                b.close()
                assert (n_local, n_whole) == ((1, 0) if sp else (0, 1))
                if r < 0:
                    continue
                d = res[sp]
                st = statistics.median(t_steady)
                d["steady"].append(st); d["act"].append(t_act); d["stall"].append(t_act - st); d["last"].append(last_ms)
                d["rest"].append(t_act - st - last_ms); d["diff"] = max(d["diff"], diff)
        for sp in (0, 1):
            d = res[sp]
            say("%8d %3d %24s %26s %26s %26s %26s %10.2f %14.3g" % (B, sp, cell(d["steady"]), cell(d["act"]), cell(d["stall"]), cell(d["last"]),
                                                                   cell(d["rest"]), statistics.median(d["stall"]) / CHUNK_MS, d["diff"]))
        sep = max(res[1]["stall"]) < min(res[0]["stall"])
        say("    %d streams: largest stall with slot_priming 1 (%.2f ms) %s the smallest with 0 (%.2f ms)" % (
            B, max(res[1]["stall"]), "is below" if sep else "IS NOT BELOW", min(res[0]["stall"])))
        say("    %d streams: device memory of the batch %.1f MiB with slot_priming 0, %.1f MiB with 1: the priming workspace takes %.1f MiB" % (
            B, mem[0], mem[1], mem[1] - mem[0]))
        stalls[B] = {sp: res[sp]["stall"] for sp in (0, 1)}
    Bm = max(streams)
    m = statistics.median(stalls[Bm][1])
    say("    goal (reported, not gated): stall at %d streams with slot_priming 1 = %.2f ms, %s one chunk period (%.1f ms x chunk)" % (
        Bm, m, "below: MET" if m < CHUNK_MS else "above: NOT MET", CHUNK_MS))
    say("    split: last_ms is the host wall time of the activation itself (prompt prefill of 33 + 2 R rows, delay fill, vocoder priming); "
        "stall - last_ms is what the activating step costs beyond a steady one outside it (draining the step before the activation)")
    say()
    return stalls


def slot_priming_b(say, E, wrap, prompt, synth_utterance, slots, repeats):
    ac, cc, style, timbre = prompt
    eng = wrap.engine
    say("(b) ragged queue of 3 x n_slots utterances of 20-120 chunks (seed 7): continuous batching (stream_infer_many, slot_priming 0 | 1) vs "
        "lock-step waves, %d repeats, the three alternating: median [min - max]" % repeats)
    say("%8s %10s %30s %30s %30s %22s %22s" % ("slots", "frames", "many sp=0 frames/s", "many sp=1 frames/s", "waves frames/s", "ratio sp=0", "ratio sp=1"))
    for n_slots in slots:
        rng = np.random.RandomState(7)
        lens = [int(x) for x in rng.randint(20, 121, size=3 * n_slots)]
        pool = [synth_utterance(1100 + i, 2048 * 120) for i in range(4)]
        srcs = [pool[i % 4][:2048 * (n - 1) + 1000] for i, n in enumerate(lens)]          # stream_infer pads each to n whole chunks
        frames = sum(lens)
        for sp in (0, 1):                                # warm-up: allocations, silence state, one restart of each kind
            wrap.stream_infer_many(srcs[:n_slots + 1], [prompt] * (n_slots + 1), n_slots=n_slots, slot_priming=bool(sp))
        fps = {0: [], 1: [], "w": []}
        for _ in range(repeats):
            for sp in (0, 1):
                t0 = time.perf_counter()
                wrap.stream_infer_many(srcs, [prompt] * len(srcs), n_slots=n_slots, slot_priming=bool(sp))
                fps[sp].append(frames / (time.perf_counter() - t0))
                n_local, n_whole, _ms = wrap.batch.activations()
                assert n_local + n_whole == len(srcs) - n_slots and (n_whole == 0 if sp else n_local == 0)
            t0 = time.perf_counter()
            for w0 in range(0, len(srcs), n_slots):
                wave = lens[w0:w0 + n_slots]
                b = E.Batch(eng, n_streams=len(wave))
                for s in range(len(wave)):
                    b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=0)
                b.begin()
                x = np.zeros((len(wave), 2048 * max(wave)), np.float32)
                for s, n in enumerate(wave):
                    a = srcs[w0 + s]
                    x[s, 2048 * n - a.shape[0]:2048 * n] = a
                for k in range(max(wave)):
                    b.step(x[:, k * 2048:(k + 1) * 2048])
                b.close()
            fps["w"].append(frames / (time.perf_counter() - t0))
        ratio = {sp: [m / w for m, w in zip(fps[sp], fps["w"])] for sp in (0, 1)}
        say("%8d %10d %30s %30s %30s %22s %22s" % (n_slots, frames, cell(fps[0], "%.1f"), cell(fps[1], "%.1f"), cell(fps["w"], "%.1f"),
                                                  cell(ratio[0]), cell(ratio[1])))
        say("    %d slots: ratio with slot_priming 1 %s the ratio with 0 (medians %.2f vs %.2f; %d restarts per run)" % (
            n_slots, "is above" if statistics.median(ratio[1]) > statistics.median(ratio[0]) else "IS NOT ABOVE",
            statistics.median(ratio[1]), statistics.median(ratio[0]), len(srcs) - n_slots))
    say("    (all sides step synchronously through host buffers; a wave runs max(len) steps with its finished slots idle)")
    say()


def twin_pcm_lines(say, path):
    import xml.etree.ElementTree as ET

    say("twin PCM: largest |restarted slot - twin| over the compared chunks, per vocoder-state form (tests/test_gpu_slot_priming.py, recorded properties)")
    for tc in ET.parse(path).getroot().iter("testcase"):
        props = {p.get("name"): p.get("value") for p in tc.iter("property")}
        for k in sorted(props):
            if k.startswith("pcm_max_abs_diff"):
                say("    %-70s %-24s %.3g   bit-equal: %s" % (tc.get("name"), k, float(props[k]), props.get(k.replace("pcm_max_abs_diff", "pcm_bit_equal"))))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--slot-priming", action="store_true", help="A/B arm: parts (a) and (b) for slot_priming 0 and 1, alternating per repeat")
    ap.add_argument("--twin-pcm", default=None, help="junit xml of tests/test_gpu_slot_priming.py: its recorded twin-PCM differences go into the report")
    ap.add_argument("--streams", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="built checkout of the parent commit for part (c)")
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b", "c"])
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "slot_priming_report.txt" if args.slot_priming else "stream_restart_report.txt")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if "a" not in args.skip or "b" not in args.skip:
        import torch
        torch.set_grad_enabled(False)
        from oracle import sva_oracle as O
        from streamvoiceanon_amd import engine as E, specs
        from streamvoiceanon_amd.infer_arvc import InferenceWrapper
        from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

        W = O.load_synth_weights(0, specs.all_specs(prompt_path=True))
        wrap = InferenceWrapper(weights=W)
        eng = wrap.engine
        prompt = synth_prompt(2000, 107)
        ac, cc, style, timbre = prompt

    if args.slot_priming:
        if "a" not in args.skip:
            slot_priming_a(say, E, eng, prompt, synth_utterance, args.streams, args.repeats)
            flush()
        if "b" not in args.skip:
            slot_priming_b(say, E, wrap, prompt, synth_utterance, args.slots, args.repeats)
            flush()
        if "a" not in args.skip or "b" not in args.skip:
            wrap.close()
            eng.close()
        if args.twin_pcm:
            twin_pcm_lines(say, args.twin_pcm)
            flush()
        args.skip = list(args.skip) + ["a", "b"]

    stall_ms = {}
    # ---- (a) -------------------------------------------------------------------------------------------------------------------
    if "a" not in args.skip:
        say("(a) sva_stream_restart and the activating step, chunk 1, delay 2, prompt 107 frames: median of %d restarts (ms, wall, synchronised steps)" % args.repeats)
        say("%8s %12s %14s %16s %12s %22s %s" % ("streams", "restart()", "steady step", "activating step", "stall", "stall / chunk period", "twin PCM bit-equal"))
        for B in args.streams:
            b = E.Batch(eng, n_streams=B)
            for s in range(B):
                b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=1000)
            b.begin()
            utt = synth_utterance(1000, 2048 * 12)
            src = np.repeat(utt[None], B, 0)
            t_restart, t_act, t_steady, bit_equal = [], [], [], True
            first = [b.step(src[:, k * 2048:(k + 1) * 2048])[0].copy() for k in range(12)]            # slot 0 from the batch's start: the twin
            for r in range(args.repeats):
                slot = B - 1
                b.sync()
                t0 = time.perf_counter()
                b.restart(slot, cc, ac, style, timbre, noise_seed=1000)
                t_restart.append((time.perf_counter() - t0) * 1e3)
                for k in range(12):
                    x = src[:, k * 2048:(k + 1) * 2048]
                    t0 = time.perf_counter()
                    y = b.step(x)
                    dt = (time.perf_counter() - t0) * 1e3
                    (t_act if k == 1 else t_steady).append(dt)       # delay 2: the slot activates at the end of its second step
                    bit_equal = bit_equal and np.array_equal(y[slot], first[k])
            b.close()
            st, act = statistics.median(t_steady), statistics.median(t_act)
            say("%8d %12.2f %14.2f %16.2f %12.2f %22.2f %s" % (B, statistics.median(t_restart), st, act, act - st, (act - st) / CHUNK_MS, bit_equal))
            stall_ms[B] = act - st
            if B == max(args.streams):
                over = (act - st) > CHUNK_MS
                say("    stall at %d streams %s one chunk period (%.1f ms x chunk)%s" % (
                    B, "EXCEEDS" if over else "is below", CHUNK_MS,
                    ": follow-up = a one-slot vocoder priming path (prime the slot's state in a 1-stream run instead of the whole batch)" if over else ""))
        say()
        flush()

    # ---- (b) -------------------------------------------------------------------------------------------------------------------
    if "b" not in args.skip:
        say("(b) ragged queue of 3 x n_slots utterances of 20-120 chunks (seed 7): continuous batching (stream_infer_many) vs lock-step waves")
        say("%8s %10s %14s %16s %16s %8s" % ("slots", "frames", "steps many", "many frames/s", "waves frames/s", "ratio"))
        for n_slots in args.slots:
            rng = np.random.RandomState(7)
            lens = [int(x) for x in rng.randint(20, 121, size=3 * n_slots)]
            pool = [synth_utterance(1100 + i, 2048 * 120) for i in range(4)]
            srcs = [pool[i % 4][:2048 * (n - 1) + 1000] for i, n in enumerate(lens)]          # stream_infer pads each to n whole chunks
            frames = sum(lens)
            steps = []
            wrap.stream_infer_many(srcs[:n_slots], [prompt] * n_slots, n_slots=n_slots)         # warm-up: allocations, silence state, tuning
            t0 = time.perf_counter()
            wrap.stream_infer_many(srcs, [prompt] * len(srcs), n_slots=n_slots, on_step=lambda k, f: steps.append(k))
            t_many = time.perf_counter() - t0
            t0 = time.perf_counter()
            for w0 in range(0, len(srcs), n_slots):
                wave = lens[w0:w0 + n_slots]
                b = E.Batch(eng, n_streams=len(wave))
                for s in range(len(wave)):
                    b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=0)
                b.begin()
                x = np.zeros((len(wave), 2048 * max(wave)), np.float32)
                for s, n in enumerate(wave):
                    a = srcs[w0 + s]
                    x[s, 2048 * n - a.shape[0]:2048 * n] = a
                for k in range(max(wave)):
                    b.step(x[:, k * 2048:(k + 1) * 2048])
                b.close()
            t_waves = time.perf_counter() - t0
            say("%8d %10d %14d %16.1f %16.1f %8.2f" % (n_slots, frames, len(steps), frames / t_many, frames / t_waves, t_waves / t_many))
            n_re = len(srcs) - n_slots
            if n_slots in stall_ms:
                say("    %d slots: %d restarts x %.0f ms stall (a) = %.1f s of the %.1f s continuous run (waves: %.1f s) -> continuous batching %s" % (
                    n_slots, n_re, stall_ms[n_slots], n_re * stall_ms[n_slots] * 1e-3, t_many, t_waves,
                    "wins" if t_many < t_waves else "LOSES to lock-step waves while a restart stalls the whole batch; the one-slot priming path is what it needs"))
        say("    (both sides step synchronously through host buffers; a wave runs max(len) steps with its finished slots idle)")
        say()
        flush()
        wrap.close()
        eng.close()

    # ---- (c) -------------------------------------------------------------------------------------------------------------------
    if "c" not in args.skip:
        say("(c) bench.py frames/s, %d runs each, the two trees alternating" % args.bench_runs)
        trees = [("this change", ROOT)] + ([("parent", args.parent_root)] if args.parent_root else [])
        if not args.parent_root:
            say("    (no --parent-root given: this tree only)")
        for extra in ([], ["--streams", "64"]):
            res = {name: [] for name, _ in trees}
            for _ in range(args.bench_runs):
                for name, root in trees:
                    p = subprocess.run([sys.executable, "bench.py"] + extra, cwd=root, capture_output=True, text=True)
                    val = None
                    for ln in p.stdout.splitlines():
                        if ln.startswith("{"):
                            try:
                                val = json.loads(ln).get("value", val)
                            except ValueError:
                                pass
                    if val is None:
                        say("    bench.py %s failed in %s (rc %d): %s" % (" ".join(extra), name, p.returncode, p.stderr.strip()[-300:]))
                    else:
                        res[name].append(float(val))
            for name, _ in trees:
                v = res[name]
                if v:
                    say("    bench.py %-14s %-12s runs %s  median %.1f  min %.1f" % (" ".join(extra) or "(default)", name, ["%.1f" % x for x in v], statistics.median(v), min(v)))
            if args.parent_root and res["this change"] and res["parent"]:
                ok = statistics.median(res["this change"]) >= min(res["parent"])
                say("    median of this change %s the lowest of the parent's runs" % ("is not below" if ok else "IS BELOW"))
        flush()
    flush()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
