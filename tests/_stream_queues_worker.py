"""Worker of tests/test_gpu_stream_queues.py: one fresh process with the queue pool pinned by its parent (GPU_MAX_HW_QUEUES=4).  It
imports torch and allocates a tensor first, as a host application would, then builds one engine and prints one JSON line:
  overlap   {case: {pair: bool}} of Batch.stream_overlap() for a pipelined batch at 1 stream (persistent decode), at 8 streams (batched
            persistent decode, unpartitioned) and at 8 streams with SVA_DEBUG cu_partition=1 (CU-masked streams)
  equal     {B: {what: bool}}: 12 pipelined chunks against the same 12 chunks stepped synchronously, bit for bit
  paths     decode path of the three batches"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_CHUNKS = 12


def run(E, eng, chunks, B, pipeline, taps):
    """12 chunk-steps of B seeded streams -> (pcm [chunks, B, 2048], audio codes [B, 8, frames], content codes [chunks, B] or None)"""
    import torch
    from streamvoiceanon_amd.synth_audio import synth_prompt

    b = E.Batch(eng, n_streams=B, pipeline=pipeline)
    for i in range(B):
        ac, cc, style, timbre = synth_prompt(2950 + i % 3, 40 + 10 * (i % 3))
        b.prefill_prompt(i, cc, ac, style, timbre, noise_seed=600 + i)
    b.begin()
    out = torch.zeros(N_CHUNKS, B, 2048, device="cuda")
    content = []
    for k in range(N_CHUNKS):
        b.step_device_on(chunks[k].data_ptr(), out[k].data_ptr(), join_output=False)
        if taps:            # (a tap drains the pipeline: the run without taps is the one whose steps overlap)
            content.append(b.tap("content_codes", (B, 1), np.int32)[:, 0].copy())
    b.join_stream()
    res, codes = out.cpu().numpy(), np.stack([b.pred_codes(i) for i in range(B)])
    b.close()
    return res, codes, np.stack(content) if taps else None


def main():
    import torch

    host = torch.ones(1024, device="cuda")          # the host application's own work comes first: its streams hold their queues
    torch.cuda.synchronize()

    from streamvoiceanon_amd import engine as E, specs, synth_weights
    from streamvoiceanon_amd.synth_audio import synth_utterance

    eng = E.Engine(synth_weights.generate_all(0, specs.all_specs()))
    lib = E.load_library()
    res = {"overlap": {}, "equal": {}, "paths": {}, "queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    for case, B, debug in (("b1", 1, None), ("b8", 8, None), ("b8_cu_partition", 8, b"cu_partition=1")):
        if debug:
            lib.sva_debug_configure(debug)           # read when a batch is created
        try:
            b = E.Batch(eng, n_streams=B, chunk_frames=1, pipeline=True)
        finally:
            if debug:
                lib.sva_debug_configure(b"cu_partition=-1")
        res["paths"][case] = b.decode_path()
        res["overlap"][case] = b.stream_overlap()
        b.close()
    for B in (1, 8):
        audio = torch.from_numpy(np.stack([synth_utterance(7700 + i % 4, 2048 * N_CHUNKS) for i in range(B)])).cuda()
        chunks = audio.reshape(B, N_CHUNKS, 2048).transpose(0, 1).contiguous()
        pcm_s, codes_s, content_s = run(E, eng, chunks, B, False, True)
        pcm_p, codes_p, _ = run(E, eng, chunks, B, True, False)
        pcm_t, codes_t, content_t = run(E, eng, chunks, B, True, True)
        res["equal"][str(B)] = {
            "pcm_nonzero": bool(np.abs(pcm_s[3:]).max() > 1e-3),
            "pcm": bool(np.array_equal(pcm_s, pcm_p) and np.array_equal(pcm_s, pcm_t)),
            "audio_codes": bool(codes_s.shape[-1] > 0 and np.array_equal(codes_s, codes_p) and np.array_equal(codes_s, codes_t)),
            "content_codes": bool(np.array_equal(content_s, content_t)),
        }
    eng.close()
    assert float(host.sum()) == 1024.0
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
