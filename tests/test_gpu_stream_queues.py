"""The four chains of the pipelined step (main, encoder side, AR, vocoder) each get a hardware queue of their own with the runtime's
queue pool at 4 entries and a host application (torch) already holding its share -- csrc/engine.hip get_streams -- and the results do
not depend on it.  One fresh child process (the pool size is read when the HIP runtime starts) serves every test of this file."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CASES = ("b1", "b8", "b8_cu_partition")


@pytest.fixture(scope="module")
def worker_result():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_stream_queues_worker.py")
    env = dict(os.environ)
    env.pop("SVA_DEBUG", None)
    env["GPU_MAX_HW_QUEUES"] = "4"          # never below 4: graph replay with parallel branches needs them
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-500:]
    res = json.loads(line[-1][len("RESULT "):])
    print(json.dumps(res, indent=1))
    assert res["queues"] == "4"
    return res


@pytest.mark.parametrize("case", CASES)
def test_chain_streams_run_concurrently_with_a_pool_of_four(worker_result, case):
    """1 stream (persistent decode), 8 streams (batched persistent decode, unpartitioned), 8 streams on CU-masked streams: a kernel
    enqueued on any of the four streams starts while a kernel enqueued earlier on any other of them is still running."""
    assert worker_result["paths"] == {"b1": 1, "b8": 2, "b8_cu_partition": 2}
    pairs = worker_result["overlap"][case]
    assert len(pairs) == 6
    assert all(pairs.values()), f"{case}: streams that share a hardware queue: {[p for p, ok in pairs.items() if not ok]}"


@pytest.mark.parametrize("B", [1, 8])
def test_pipelined_equals_serial_with_a_pool_of_four(worker_result, B):
    """12 pipelined chunks (overlapped, and with a tap after every chunk) = the same 12 chunks stepped synchronously, bit for bit:
    content codes, audio codes, PCM."""
    eq = worker_result["equal"][str(B)]
    assert eq == {"pcm_nonzero": True, "pcm": True, "audio_codes": True, "content_codes": True}
