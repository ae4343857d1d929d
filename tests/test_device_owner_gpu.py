"""GPU: what the three handles (ch_model, ch_trainer, ch_text) own through csrc/device_owner.h.  Reported bytes equal the parent
commit's, handles that are created and closed give all device memory back, and the staging buffers of the hipGraph replay path grow by
release-then-alloc (model.hip ensure_bytes) by exactly the derived amount.  Allocation FAILURE is tested on the CPU
(tests/test_device_owner_cpu.py); nothing here provokes one."""
import gc

import numpy as np
import pytest
import torch

import text_tower_ref as ttr
from test_text_tower_gpu import SMALL, B as TEXT_B, small_ids

pytestmark = pytest.mark.gpu

# ch_model_device_bytes of synthetic ViT-B/16 (12 layers), nbit 64, nclass 10, max_batch 32, default options, and ch_text_device_bytes of the
# two-layer tower of tests/test_text_tower_gpu.py (max_batch 3): each measured with the parent commit's library and with this one's
MODEL_BYTES_B16_BATCH32 = 472382816     # parent commit: 472,382,816; this commit: 472,382,816
TEXT_BYTES_SMALL_TOWER = 1920424         # parent commit: 1,920,424; this commit: 1,920,424


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def small_vit():
    """the 3-layer ViT-S/16 of test_graph_replay_of_small_batches_is_bit_identical"""
    from oracle import encoder_oracle as eo
    cfg = dict(eo.CONFIGS["vit_s16"])
    cfg["L"] = 3
    return cfg, eo.synthetic_state_dict(cfg, nbit=64, nclass=10)


def _encoder(sd, heads, **kw):
    from concepthash_amd.encoder import ConceptHashEncoder
    return ConceptHashEncoder(sd, heads=heads, **kw)


def test_reported_bytes_of_model_and_text_handles_did_not_move(dev):
    from concepthash_amd import synthetic
    from concepthash_amd.text import TextEncoder
    cfg = dict(synthetic.CONFIGS["vit_b16"])
    enc = _encoder(synthetic.synthetic_state_dict(cfg, nbit=64, nclass=10, seed=3), cfg["heads"], max_batch=32, device=dev)
    model_bytes = enc.device_bytes
    enc.close()
    txt = TextEncoder(SMALL, ttr.seeded_text_state_dict(SMALL, seed=1), max_batch=TEXT_B)
    text_bytes = txt.device_bytes
    txt.close()
    print(f"ch_model_device_bytes ViT-B/16 batch 32: {model_bytes}; ch_text_device_bytes 128 x 2 tower, batch {TEXT_B}: {text_bytes}")
    assert model_bytes == MODEL_BYTES_B16_BATCH32
    assert text_bytes == TEXT_BYTES_SMALL_TOWER


def test_closed_handles_give_all_device_memory_back(dev, small_vit):
    """One cycle creates, uses and closes an encoder (an encode and a profiled encode: the profiler's events), a TrainEngine (a forward and
    a backward: the aux stream and the fork / join events) and a TextEncoder (the pinned staging buffer and its event).  After a warm-up
    cycle (code objects, the runtime's own pools), free device memory after cycles 2 and 3 equals that after cycle 1.  A leak check: it
    provokes nothing."""
    from concepthash_amd.text import TextEncoder
    from concepthash_amd.training import TrainEngine, adapters_from_state_dict
    from oracle import encoder_oracle as eo
    cfg, sd = small_vit
    x = eo.synthetic_images(8, cfg["image"]).to(dev)
    ctx = eo.concept_tokens(sd, 8)[0].to(dev)
    tsd = ttr.seeded_text_state_dict(SMALL, seed=1)
    ids, eos = small_ids(16), np.array([15, 8, 0], dtype=np.int32)

    def cycle():
        enc = _encoder(sd, cfg["heads"], max_batch=8, device=dev)
        enc.encode(x)
        enc.profile_begin(enc.launches_per_encode + 10)
        enc.encode(x)
        torch.cuda.synchronize()
        enc.profile_end()
        enc.close()
        eng = TrainEngine(sd, adapters_from_state_dict(sd, cfg["L"], cfg["D"], cfg["b"]), heads=cfg["heads"], max_batch=8, device=dev)
        hf, _ = eng.forward(x, ctx)
        eng.backward(torch.ones_like(hf))
        torch.cuda.synchronize()
        eng.close()
        txt = TextEncoder(SMALL, tsd, max_batch=TEXT_B)
        txt.encode_batch(ids, eos)
        torch.cuda.synchronize()
        txt.close()
        del enc, eng, txt, hf
        gc.collect()
        free = []
        for _ in range(3):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free.append(torch.cuda.mem_get_info(dev)[0])
        return min(free)

    cycle()   # warm-up
    free = [cycle() for _ in range(3)]
    print(f"free device bytes after cycles 1..3: {free}; drift {[free[0] - f for f in free[1:]]}")
    assert free[1] == free[0] and free[2] == free[0], free


def test_graph_staging_buffers_regrow_by_the_derived_amount(dev, small_vit):
    """graph_max_batch 2 -> 8 on one handle: the fp32 input staging and every requested output's staging buffer are released and allocated
    again at the larger capacity.  Outputs stay bit-equal to an eager encoder's through capture and replay at both sizes, and device_bytes
    grows by six images' worth of each: 6 * 3 * image^2 * 4 for the input, and per image 4 * nbit (codes), 8 * ceil(nbit / 64) (packed),
    4 * Q * D (hash_features), as encode_graph's out_bytes.  (8 * ntok rows: the one-chain path, as the replay test above.)"""
    from oracle import encoder_oracle as eo
    cfg, sd = small_vit
    want = ("codes", "packed", "hash_features")
    x = eo.synthetic_images(8, cfg["image"]).to(dev)
    eager = _encoder(sd, cfg["heads"], max_batch=8, options={"graph_max_batch": 0})
    graph = _encoder(sd, cfg["heads"], max_batch=8, options={"graph_max_batch": 2})
    ref = {B: eager.encode(x[:B], want=want) for B in (2, 8)}
    sizes = []
    for B in (2, 8):
        graph.set_option("graph_max_batch", B)
        for rep in range(2):   # capture, then replay
            got = graph.encode(x[:B], want=want)
            torch.cuda.synchronize()
            for k in want:
                assert torch.equal(got[k], ref[B][k]), (B, rep, k)
        sizes.append(graph.device_bytes)
    c = graph.cfg
    per_image = 3 * c["image_size"] ** 2 * 4 + 4 * c["nbit"] + 8 * ((c["nbit"] + 63) // 64) + 4 * c["ncontext"] * c["dim"]
    print(f"device_bytes with staging for 2 / 8 images: {sizes}; growth {sizes[1] - sizes[0]}, derived {6 * per_image}")
    assert sizes[1] - sizes[0] == 6 * per_image
    assert graph.get_option("graph_captures") == 2 and graph.get_option("graph_replays") == 2
    assert eager.device_bytes == sizes[0] - 2 * per_image
    eager.close()
    graph.close()
