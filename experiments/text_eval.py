"""`RetrievalEvaluation` that also scores the run's class prompts as text queries: config keys `text_eval: true`, `prompt_prefix`,
`text_model` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  The queries are the C class
prompts -- `trainers.orthohash.class_prompts` of the dataset's class_names.txt under the run's prompt prefix -- turned into codes as
`exp=search query=classes` turns them ("text query": text tower, centre row, the model's own text_projection),
with label = class id.  They are scored against the database codes the evaluator has already encoded and post-processed, through the
`calculate_mAP` call the image queries of the whole code went through, with its R, PRs, threshold and metric: `mAP_text`,
`recalls_text`, `precisions_text` and `center_agreement` are added to the results and to `history.json`.  The text codes are never shifted
by the database mean (`zero_mean_eval` shifts the database side only).  Cost: one text-tower batch and one C-query scan.  It extends
the asymmetric, hash-lookup, concept and tie-bracket evaluators, so their keys keep working beside it.
"""
from __future__ import annotations

import json
import os

import torch

import experiments.test_hashing as base
import utils.hashing
from experiments.asymmetric_eval import AsymmetricEvaluation
from experiments.search import class_name_file

KEYS = ("mAP_text", "recalls_text", "precisions_text")
# what a wrapped evaluator adds to a call for its own bookkeeping, and what only makes sense when the queries are database rows
NOT_FOR_TEXT = ("tie_bracket", "tie_expected", "radii", "remove_first_retrieved", "rank", "weight_bits")


def text_eval_request(config):
    """(text model directory, prefix, class_names.txt, the run's own prefix) of a `text_eval` run, from its config alone; every argument error of the key is
    raised here, before a model is built or a GPU touched."""
    import torch.distributed as dist
    from concepthash_amd.text import text_query_settings
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("text_eval under a multi-rank process group is not built (sharded text queries are out of scope); "
                                  "run the evaluation with text_eval as a single process")
    if not config.get("compute_mAP") or config.exp == "extract":
        raise ValueError("text_eval scores the class prompts by mAP / P@k / R@k: it needs compute_mAP=True and exp=validation")
    for key in ("sub_code_eval", "test_as_database"):
        if config.get(key):
            raise ValueError(f"text_eval scores the class prompts against the whole code of the database split; it cannot be combined with {key}")
    source, prefix = text_query_settings(config, config.get("text_model"), config.get("prompt_prefix"))
    names = class_name_file(config)
    if not os.path.isfile(names):
        raise ValueError(f"text_eval reads one class name per line from {names}, which does not exist")
    return source, prefix, names, text_query_settings(config, config.get("text_model"))[1]


class TextEvaluation(AsymmetricEvaluation):
    def __init__(self, config):
        self.text = text_eval_request(config) if config.get("text_eval") else None
        super().__init__(config)

    def main(self):
        cfg = self.config
        if getattr(self, "text", None) is None:
            return super().main()
        source, prefix, names, run_prefix = self.text
        nbit = int(cfg.model.nbit)
        metric, name = utils.hashing.calculate_mAP, base.calculate_mAP
        whole = []                         # the evaluator's Hamming calls on the whole code: (db_codes, db_labels, R, keyword arguments)

        def recording(db_codes, db_labels, test_codes, test_labels, R, **k):
            if int(db_codes.shape[1]) == nbit and k.get("rank", "hamming") == "hamming":
                whole.append((db_codes, db_labels, R, {key: v for key, v in k.items() if key not in NOT_FOR_TEXT}))
            return metric(db_codes, db_labels, test_codes, test_labels, R, **k)
        # The innermost name, as the hash-lookup evaluator wraps it: every evaluator above ends up in `utils.hashing.calculate_mAP`.
        utils.hashing.calculate_mAP = base.calculate_mAP = recording
        try:
            res = super().main()
        finally:
            utils.hashing.calculate_mAP, base.calculate_mAP = metric, name
        if not whole:
            raise RuntimeError(f"text_eval: the evaluator made no calculate_mAP call on the whole {nbit}-bit code")
        db_codes, db_labels, R, kw = whole[-1]
        from concepthash_amd.text import TextQueryEncoder
        from trainers.orthohash import class_prompts
        model = self.trainer.model
        model.eval()
        prompts = class_prompts(names, prefix)
        if len(prompts) != int(cfg.dataset.nclass):
            raise ValueError(f"{names} names {len(prompts)} classes, the dataset has {cfg.dataset.nclass}")
        with TextQueryEncoder(model, source, prefix="") as enc, torch.no_grad():     # the prompts carry their prefix
            text_codes = self._phase("encode_text", enc.text_codes, prompts).cpu()
            res["center_agreement"] = enc.center_agreement(names, run_prefix)     # the tower check: the run's own prefix
        text_labels = torch.eye(len(prompts), dtype=db_labels.dtype)
        left = utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup, utils.hashing.last_tie_expected      # what the evaluators above read stays the image queries'
        out = self._phase("retrieval_text", metric, db_codes, db_labels, text_codes, text_labels, R, **kw)
        utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup, utils.hashing.last_tie_expected = left
        for key, v in zip(KEYS, out):
            res[key] = v
        res["text_prompt_prefix"], res["text_model"] = prefix, source
        if isinstance(res.get("timing_s"), dict):
            res["timing_s"].update({key: self.timing[key] for key in ("encode_text", "retrieval_text")})
        many = isinstance(out[0], list)
        for r_, m in (zip(R, out[0]) if many else [(R, out[0])]):
            print(f"mAP@{r_} (text: {len(prompts)} class prompts): {m:.4f}")
        for kk, r, p in zip(kw.get("PRs") or [], out[1], out[2]):
            print(f"P@{kk} (text): {p:.4f}; R@{kk} (text): {r:.4f}")
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
