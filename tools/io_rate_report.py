"""What the I/O adaptor (include/sva.h: sva_io_*) costs -> profiles/io_rate_report.txt.

    python tools/io_rate_report.py [--out profiles/io_rate_report.txt]

Per configuration (48 kHz float32, 16 kHz int16) and per batch size (1, 8, 64 streams), on the device this runs on:
  * the period of one engine step of a pipelined batch stepped through sva_io_process_device, against the same batch type stepped with
    sva_step_device and no adaptor -- host clock around a window of about 1.5 s of steps that ends in a synchronise, three repeats each,
    alternated;
  * the stand-alone time of the two kernels per engine step, from a rocprofv3 --kernel-trace --stats run of the adaptor loop alone (a child
    process of its own: tracing slows the host, so no period is taken there);
  * L in milliseconds;
  * the host path the adaptor replaces: audio_io.resample in and out for one chunk of every stream, on this machine's CPU.
Needs an MI355X; fails without one.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = ((48000, "f32"), (16000, "i16"))
STREAMS = (1, 8, 64)
TIMED_SECONDS = 1.5        # each timed window runs about this long: at one stream a step is under a millisecond, and a window of a fraction of
                           # a second would measure the clock and the scheduler as much as the step
REPEATS = 3
MODEL = 44100


def make_engine():
    from streamvoiceanon_amd import engine as E, specs, synth_weights

    return E.Engine(synth_weights.generate_all(0, specs.all_specs()), device=0)


def make_batch(eng, B):
    from streamvoiceanon_amd import engine as E
    from streamvoiceanon_amd.synth_audio import synth_prompt

    b = E.Batch(eng, n_streams=B, chunk_frames=1, delay=2, pipeline=True, skip_semantic=True)
    for s in range(B):
        ac, cc, style, timbre = synth_prompt(2000 + s, 107)
        b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=1000 + s)
    b.begin()
    return b


def source(B, n, dtype):
    from streamvoiceanon_amd.synth_audio import synth_utterance

    x = np.stack([synth_utterance(1000 + s, n) for s in range(B)])
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def plain_period(eng, B, steps, warmup=12):
    """ms per sva_step_device step of a pipelined batch, no adaptor"""
    import torch

    b = make_batch(eng, B)
    x = torch.from_numpy(source(B, 2048 * 8, np.float32)).cuda().reshape(B, 8, 2048).transpose(0, 1).contiguous()
    out = torch.empty(B, 2048, device="cuda")
    torch.cuda.synchronize()
    for k in range(warmup):
        b.step_device(x[k % 8].data_ptr(), out.data_ptr())
    b.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        b.step_device(x[k % 8].data_ptr(), out.data_ptr())
    b.sync()
    dt = time.perf_counter() - t0
    b.close()
    return dt / steps * 1e3


def adaptor_loop(eng, B, rate, fmt, steps, warmup=12):
    """-> (ms per engine step through sva_io_process_device, L in samples, block length): blocks of one chunk's worth of samples at `rate`"""
    import torch
    from streamvoiceanon_amd import engine as E

    b = make_batch(eng, B)
    block = int(round(2048 * rate / MODEL))
    io = b.open_io(rate, fmt, max_block=block)
    dtype = E.IO_FORMATS[fmt][1]
    x = torch.from_numpy(source(B, block * 8, dtype)).cuda().reshape(B, 8, block).transpose(0, 1).contiguous()
    out = torch.empty(B, block, device="cuda", dtype=x.dtype)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    _, rows = E.test_io_plan(rate, 1, [block] * (warmup + steps))
    for k in range(warmup):
        io.process_device(x[k % 8].data_ptr(), out.data_ptr(), block, stream=stream, join_output=False)
    b.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        io.process_device(x[k % 8].data_ptr(), out.data_ptr(), block, stream=stream, join_output=False)
    b.sync()
    dt = time.perf_counter() - t0
    n_steps = int(rows[warmup:, 1].sum())
    L = io.latency
    b.close()
    return dt / max(n_steps, 1) * 1e3, L, block


def worker(rate, fmt, B, steps):
    """the adaptor loop alone, for the kernel trace"""
    eng = make_engine()
    adaptor_loop(eng, B, rate, fmt, steps)
    eng.close()


def kernel_times(rate, fmt, B, steps, scratch):
    """-> {kernel: (calls, average us)} of the two adaptor kernels, from a traced child process"""
    d = os.path.join(scratch, f"trace_{rate}_{fmt}_{B}")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
           "--worker", str(rate), fmt, str(B), "--steps", str(steps)]
    env = dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp"))
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"traced worker failed ({r.returncode}): {r.stdout[-2000:]}")
    found = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in ("io_resample_in_kernel", "io_resample_out_kernel"):
                if k in row["Name"]:
                    found[k] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    shutil.rmtree(d, ignore_errors=True)
    return found


def host_path_ms(rate, B, repeats=5):
    """audio_io.resample of one chunk of B streams, in and out, ms (best of `repeats`)"""
    from streamvoiceanon_amd import audio_io

    block = int(round(2048 * rate / MODEL))
    x = source(B, block, np.float32)
    y = source(B, 2048, np.float32)
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        audio_io.resample(x, rate, MODEL)
        audio_io.resample(y, MODEL, rate)
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="timed steps per window (default: as many as fill TIMED_SECONDS, from a 50-step probe)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "io_rate_report.txt"))
    ap.add_argument("--scratch", default=None, help="directory for the traces of the child runs (default: a temporary one, removed at the end)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child runs (kernel times are then reported as not measured)")
    ap.add_argument("--worker", nargs=3, metavar=("RATE", "FMT", "B"), default=None, help="(internal) the adaptor loop alone")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("io_rate_report: no GPU visible; nothing here can be measured without one")
    if args.worker:
        return worker(int(args.worker[0]), args.worker[1], int(args.worker[2]), args.steps)
    scratch = args.scratch or tempfile.mkdtemp(prefix="io_rate_report_")
    os.makedirs(scratch, exist_ok=True)
    eng = make_engine()
    lines = ["I/O adaptor: cost per engine step (tools/io_rate_report.py)",
             f"device: {torch.cuda.get_device_name(0)}; pipelined batches, chunk_frames 1, 12 warm-up steps before every timed window, device RNG",
             f"period = host clock around the timed steps, ending in a synchronise, per engine step; {REPEATS} repeats, alternated plain / adaptor;",
             f"         timed steps per window: {args.steps or 'about %.1f s worth' % TIMED_SECONDS} (stated per row)",
             "kernels = rocprofv3 --kernel-trace --stats of the adaptor loop in a child process: average time of one launch (one launch of each",
             "          per engine step at these block lengths, which are one chunk's worth of samples at the rate)",
             ""]
    for rate, fmt in CONFIGS:
        for B in STREAMS:
            steps = args.steps or max(200, int(TIMED_SECONDS * 1e3 / plain_period(eng, B, 50)))
            plain, adapt = [], []
            for _ in range(REPEATS):
                plain.append(plain_period(eng, B, steps))
                a, L, block = adaptor_loop(eng, B, rate, fmt, steps)
                adapt.append(a)
            kt = {} if args.no_trace else kernel_times(rate, fmt, B, 200, scratch)
            ktxt = ("in %.1f us + out %.1f us = %.1f us per step (%d / %d launches traced)" % (
                kt["io_resample_in_kernel"][1], kt["io_resample_out_kernel"][1], kt["io_resample_in_kernel"][1] + kt["io_resample_out_kernel"][1],
                kt["io_resample_in_kernel"][0], kt["io_resample_out_kernel"][0])) if len(kt) == 2 else "not measured"
            host = host_path_ms(rate, B)
            fmt3 = lambda v: " / ".join("%.4f" % t for t in v)
            lines += [f"{rate} Hz {fmt}, {B} stream(s), blocks of {block} samples, {steps} timed steps per window:",
                      f"  period without adaptor  {fmt3(plain)} ms per step",
                      f"  period with adaptor     {fmt3(adapt)} ms per step   (difference of the means {1e3 * (np.mean(adapt) - np.mean(plain)):+.1f} us; "
                      f"spread of the repeats {1e3 * (max(plain) - min(plain)):.1f} / {1e3 * (max(adapt) - min(adapt)):.1f} us)",
                      f"  kernels                 {ktxt}",
                      f"  L                       {L} samples = {1e3 * L / rate:.2f} ms",
                      f"  host path replaced      audio_io.resample in + out for one chunk of {B} stream(s): {host:.3f} ms on this machine's CPU (one BLAS thread), "
                      "plus two host<->device copies per chunk, not timed here",
                      ""]
            print("\n".join(lines[-7:]), flush=True)
    eng.close()
    if args.scratch is None:
        shutil.rmtree(scratch, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
