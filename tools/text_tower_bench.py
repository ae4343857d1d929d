"""Time of `ch_text_encode` for 200 x 77 prompts on CLIP ViT-B's text tower (512 x 12, full vocabulary, seeded weights; DESIGN.md
section 3.12): HIP events around the whole call, warmed, median of several.  Beside it a torch fp32 run of the TEST RESTATEMENT
(tests/text_tower_ref.py) on the same GPU -- not the reference.  `python tools/text_tower_bench.py [out.json]`"""
from __future__ import annotations

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIMS = dict(vocab_size=49408, max_position_embeddings=77, hidden_size=512, num_hidden_layers=12, num_attention_heads=8, intermediate_size=2048)
EOS = 49407
PROMPTS, BATCH = 200, 100


def timed(fn, n=9, warm=3):
    """(median, min, max) ms of n calls after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        ts.append(start.elapsed_time(stop))
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    import text_tower_ref as ttr
    from concepthash_amd.text import TextEncoder
    sd = ttr.seeded_text_state_dict(DIMS, seed=7)
    ids = torch.randint(0, EOS, (PROMPTS, 77), generator=torch.Generator().manual_seed(8))
    ids[:, 20:] = EOS
    enc = TextEncoder(dict(DIMS, eos_token_id=EOS), sd, max_batch=BATCH)
    hip = timed(lambda: enc.encode(ids))
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    ids_gpu = ids.cuda()

    def restatement():
        return torch.cat([ttr.text_forward(sd_gpu, ids_gpu[i:i + BATCH], heads=8, eos_token_id=EOS)[1] for i in range(0, PROMPTS, BATCH)])

    with torch.no_grad():
        tor = timed(restatement)
        ref = restatement()
    d = (enc.encode(ids) - ref).double()
    prop = torch.cuda.get_device_properties(0)
    res = {"what": f"ch_text_encode, {PROMPTS} x 77 prompts ({PROMPTS // BATCH} batches of {BATCH}), CLIP ViT-B text tower 512 x 12, "
                   "full 49,408-row vocabulary, seeded weights",
           "timing": "HIP events around the whole call (host checks, id staging, launches), 3 warm-up calls, 9 timed",
           "ch_text_encode_ms": hip, "torch_fp32_test_restatement_same_gpu_ms": tor,
           "pooled_max_abs_over_rms_vs_torch_fp32_gpu": float(d.abs().max() / ref.double().pow(2).mean().sqrt()),
           "device_bytes": enc.device_bytes,
           "device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                      "memory_gib": round(prop.total_memory / 2 ** 30, 1)}}
    enc.close()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
