"""Seconds of a text query, phase by phase: tokenise / text tower / ch_model_project_text / GalleryIndex.search for
1, 100 and C = 200 prompts against a CUB-sized (5,994 rows) and a 1M-row index of 64-bit codes, with the same search on as many image-query
codes beside it for scale.  `python tools/text_query_bench.py [profiles/search_text_queries.txt]`

What is real and what is a stand-in: the text tower has CLIP ViT-B's dimensions (512 x 12, 49,408-row vocabulary) with seeded weights; the
tokeniser is the byte-level BPE of concepthash_amd/text.py over the SYNTHETIC vocabulary of tests/text_tower_ref.py (a few merges only, so a
prompt is more tokens -- the `tokens` column -- than under CLIP's 49k merges, and the tokeniser's word cache is warm in the timed calls); text_projection is
the shipped Sequential(Linear(512, 512), ReLU, Linear(512, 64)); the database codes are seeded random bits.  The tower and the projection are
timed with device events around the call, tokenise and search with a host clock around work that ends in a device synchronise; 2 warm-up
calls, median of 7."""
from __future__ import annotations

import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEXT = dict(vocab_size=49408, max_position_embeddings=77, hidden_size=512, num_hidden_layers=12, num_attention_heads=8, intermediate_size=2048)
VISION = dict(D=128, L=1, heads=2, M=256, patch=16, image=32, P=32, b=128)     # the encoder around the centre head: not timed
NBIT, NCLASS, K = 64, 200, 10
PROMPTS = (1, 100, NCLASS)
INDEX_ROWS = (("cub200 database, 5,994 rows", 5994), ("1M rows", 1_000_000))
WORDS = ("painted", "bunting", "black", "footed", "albatross", "warbler", "of", "the", "north", "red", "winged", "blackbird", "gull", "tern")


def device_ms(fn, n=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def host_ms(fn, n=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    import text_tower_ref as ttr
    from concepthash_amd import synthetic
    from concepthash_amd.encoder import ConceptHashEncoder
    from concepthash_amd.search import GalleryIndex
    from concepthash_amd.text import ClipBpeTokenizer, TextEncoder
    from trainers.orthohash import centre_rows
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as d:
        ttr.write_tokenizer_files(d)
        tok = ClipBpeTokenizer.from_directory(d)
    tower = TextEncoder(dict(TEXT, eos_token_id=TEXT["vocab_size"] - 1), ttr.seeded_text_state_dict(TEXT, seed=7), max_batch=100, device=dev)
    tok.eos_id = tok.pad_id = TEXT["vocab_size"] - 1                      # the synthetic vocabulary's ids, EOS moved to the tower's largest id
    model = ConceptHashEncoder(synthetic.synthetic_state_dict(VISION, nbit=NBIT, nclass=NCLASS, seed=3, center_dim=TEXT["hidden_size"]),
                               heads=VISION["heads"], max_batch=2, device=dev)
    g = torch.Generator().manual_seed(1)
    rows = []
    for label, G in INDEX_ROWS:
        packed, labels = synthetic.synthetic_codes(G, NBIT, seed=5, nclass=NCLASS)
        index = GalleryIndex(torch.from_numpy(packed.view("int64")).to(dev), NBIT, 4, labels=torch.from_numpy(labels).long()).to(dev)
        for n in PROMPTS:
            prompts = ["a photo of a " + " ".join(WORDS[(i + j) % len(WORDS)] for j in range(2 + i % 3)) for i in range(n)]
            ids = tok(prompts)
            feats = tower.encode(ids)
            codes = model.project_text(centre_rows(feats))
            image_codes = torch.randn(n, NBIT, generator=g).to(dev)
            res = index.search(codes, K, mean_shift=False)
            assert res["idx"].shape == (n, K) and bool((res["idx"] >= 0).all())
            rows.append({"index": label, "index_rows": G, "prompts": n, "tokens_per_prompt": int(ids.shape[1]),
                         "tokenise_ms": host_ms(lambda: tok(prompts)), "tower_ms": device_ms(lambda: tower.encode(ids)),
                         "projection_ms": device_ms(lambda: model.project_text(centre_rows(feats))),
                         "search_ms": host_ms(lambda: index.search(codes, K, mean_shift=False)),
                         "image_query_search_ms": host_ms(lambda: index.search(image_codes, K))})
        del index
    prop = torch.cuda.get_device_properties(0)
    tower.close()
    model.close()
    head = f"{'index':<28}{'prompts':>8}{'tokens':>8}{'tokenise':>10}{'tower':>10}{'project':>10}{'search':>10}{'total':>10}{'image-query search':>20}"
    lines = [__doc__.strip(), "", f"device: {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs); "
             f"nbit {NBIT}, C {NCLASS}, k {K}; seconds", "", head]
    for r in rows:
        s = {k: r[k] / 1e3 for k in ("tokenise_ms", "tower_ms", "projection_ms", "search_ms", "image_query_search_ms")}
        total = s["tokenise_ms"] + s["tower_ms"] + s["projection_ms"] + s["search_ms"]
        lines.append(f"{r['index']:<28}{r['prompts']:>8}{r['tokens_per_prompt']:>8}{s['tokenise_ms']:>10.5f}{s['tower_ms']:>10.5f}"
                     f"{s['projection_ms']:>10.5f}{s['search_ms']:>10.5f}{total:>10.5f}{s['image_query_search_ms']:>20.5f}")
    lines += ["", "json: " + json.dumps(rows)]
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
