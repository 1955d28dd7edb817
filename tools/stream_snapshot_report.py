"""Measurements of sva_stream_save / sva_stream_load -> profiles/stream_snapshot_report.txt.

  (a) save and load at 2 / 8 / 64 streams with the slot right after its activation (about 250 KV rows) and late in its window (about 1500):
      wall time of the synchronous call and its split (sva_test_snapshot_timings) into the pack / unpack kernel (hipEvents around the
      launch), the host <-> device copy of the image (wall) and the rest (wall: drain, validation, table upload, checksum, header, mirrors);
      the kernels next to one hipMemcpyDtoDAsync of the same byte count between the same events on the same stream, in the same process.
  (b) prompt reuse: the stall of the step that brings a new session into a slot -- sva_stream_restart + its activation with
      slot_priming = 1 (wall time of the activating step minus the median steady step) against sva_stream_load of a snapshot taken right
      after such an activation (wall time of the call) -- and their ratio.
  (c) headline unchanged: bench.py of this tree and of a built checkout of the parent commit (--parent-root), alternating.
Five repeats per cell, the arms alternating within one process; every cell is median [min - max].  Nothing here is a gate."""
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
N = 2048


def cell(v, fmt="%.2f"):
    return (fmt + " [" + fmt + " - " + fmt + "]") % (statistics.median(v), min(v), max(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--late-steps", type=int, default=627, help="steps before the late snapshot (about 1500 KV rows with a 107-frame prompt)")
    ap.add_argument("--parent-root", default=None, help="built checkout of the parent commit, for part (c)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b", "c"])
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import torch

    from oracle import sva_oracle as O
    from streamvoiceanon_amd import engine as E, specs
    from streamvoiceanon_amd.synth_audio import synth_prompt, synth_utterance

    torch.set_grad_enabled(False)
    eng = E.Engine(O.load_synth_weights(0, specs.all_specs()), device=0)
    prompt = synth_prompt(2801, 107)
    ac, cc, st, tm = prompt
    say("stream snapshot report: %s, %d repeats per cell, median [min - max]" % (torch.cuda.get_device_name(0), args.repeats))

    def batch(B, **kw):
        b = E.Batch(eng, n_streams=B, **kw)
        for s in range(B):
            b.prefill_prompt(s, cc, ac, st, tm, noise_seed=900 + s)
        b.begin()
        return b

    def run(b, n, src):
        x = np.zeros((b.B, N), np.float32)
        for k in range(n):
            x[:] = src[(k % 64) * N:(k % 64 + 1) * N]
            b.step(x)

    src = synth_utterance(7801, N * 64)
    if "a" not in args.skip:
        say()
        say("(a) save / load of one slot: wall ms of the synchronous call = kernel (events) + host <-> device copy + host work; D2D = hipMemcpyDtoDAsync")
        say("    of the image's byte count between the same events; kernel GB/s = image bytes read + written per kernel time, same for the copy")
        say("%7s %7s %7s %5s %20s %20s %20s %20s %20s %9s %9s" % ("streams", "KV rows", "MB", "call", "total ms", "kernel ms", "copy ms", "host ms", "D2D ms",
                                                                    "k GB/s", "D2D GB/s"))
        for B in args.streams:
            b = batch(B)
            done = 0
            for steps in (3, args.late_steps):
                run(b, steps - done, src)
                done = steps
                blob = b.save_stream(1)
                info = E.stream_blob_info(blob)
                t = {c: dict(total=[], kernel_ms=[], copy_ms=[], host_ms=[], d2d_ms=[]) for c in ("save", "load")}
                for _ in range(args.repeats):
                    for call, fn in (("save", lambda: b.save_stream(1)), ("load", lambda: b.load_stream(1, blob))):      # (load: back into its own slot, the state is unchanged)
                        t[call]["total"].append(timed(fn)[0])
                        sp = b.snapshot_timings(measure_d2d=True)
                        for k in ("kernel_ms", "copy_ms", "host_ms", "d2d_ms"):
                            t[call][k].append(sp[k])
                mb = info["payload_bytes"] / 1e6
                for call in ("save", "load"):
                    v = t[call]
                    say("%7d %7d %7.1f %5s %20s %20s %20s %20s %20s %9.0f %9.0f" % (
                        B, info["last_pos"] + 1, mb, call, cell(v["total"]), cell(v["kernel_ms"], "%.3f"), cell(v["copy_ms"]), cell(v["host_ms"]),
                        cell(v["d2d_ms"], "%.3f"), 2 * mb / statistics.median(v["kernel_ms"]), 2 * mb / statistics.median(v["d2d_ms"])))
            b.close()
    if "b" not in args.skip:
        say()
        say("(b) a new session into slot 1: restart + activation (slot_priming = 1; activating step minus the median steady step) vs load of a")
        say("    snapshot taken right after such an activation (wall time of the call); ms")
        say("%8s %14s %24s %24s %8s" % ("streams", "steady step", "restart arm: stall", "load arm: call", "ratio"))
        for B in args.streams:
            b = batch(B, slot_priming=True)
            run(b, 6, src)
            x = np.repeat(src[None, :N], B, axis=0)
            t_steady = [timed(lambda: b.step(x))[0] for _ in range(12)]
            steady = statistics.median(t_steady)
            b.restart(1, cc, ac, st, tm, noise_seed=77)
            b.step(x); b.step(x)
            blob = b.save_stream(1)                         # right after the activation: frame 0 not decoded yet
            stall, load = [], []
            for _ in range(args.repeats):
                b.restart(1, cc, ac, st, tm, noise_seed=77)
                b.step(x)
                stall.append(timed(lambda: b.step(x))[0] - steady)          # the step in which the slot's delay fills: prefill + delay fill + priming
                assert b.stream_state(1) == (2, 0)
                b.retire(1)
                load.append(timed(lambda: b.load_stream(1, blob))[0])
                assert b.stream_state(1) == (2, 0)
                b.step(x)
            say("%8d %14.2f %24s %24s %8.2f" % (B, steady, cell(stall), cell(load), statistics.median(stall) / statistics.median(load)))
            b.close()
    eng.close()
    if "c" not in args.skip and args.parent_root:
        say()
        say("(c) bench.py --gpus 1 --steps 200 --warmup 20, this tree and the parent commit's alternating, %d runs each (frames/s)" % args.bench_runs)
        res = {"parent": [], "this change": []}
        flags = ["--gpus", "1", "--steps", "200", "--warmup", "20", "--no-cpu-baseline", "--no-roofline",
               "--no-batched", "--no-torch-gpu-baseline", "--no-pmc", "--no-offline"]
        for _ in range(args.bench_runs):
            for name, root in (("parent", os.path.abspath(args.parent_root)), ("this change", ROOT)):
                out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + flags, capture_output=True, text=True, cwd=root, timeout=600)
                last = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
                if out.returncode != 0 or not last:
                    err = [ln for ln in (out.stderr or out.stdout).splitlines() if ln.strip()]
                    say("    a run of %s did not complete: %s" % (name, err[-1][:160] if err else "no output"))
                    continue
                res[name].append(float(json.loads(last[-1])["value"]))
        for name, v in res.items():
            if v:
                say("    %-12s runs %s  median %.1f [%.1f - %.1f]" % (name, ["%.1f" % x for x in v], statistics.median(v), min(v), max(v)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
