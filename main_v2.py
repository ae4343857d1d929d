#!/usr/bin/env python3
"""CLI entry point with the reference's surface (reference main_v2.py:14-64):

    python main_v2.py --config-name val.yaml logdir=<run dir> dataset=cub200 [R=-1] [PRs=[1,5,10]] [batch_size=64] ...
    python main_v2.py exp=extract model=concept_hash_final_v1_nosa_apt dataset=synthetic_cub200 ...
    python main_v2.py --config-name search.yaml logdir=<run dir> dataset=cub200 [query=test] [k=10] [radius=2] [concepts=[0,2]] [rotate=itq] [reduce=pca-itq reduce_bits=32] ...

`exp` dispatch: hashing -> RetrievalExperiment (train the adapters + hashing head, frozen backbone); validation -> load
<logdir>/config.yaml, overlay the evaluation knobs, RetrievalEvaluation; search -> the same run config, SearchExperiment (ranked hits of
image or text queries, experiments/search.py); descriptor / extract -> RetrievalEvaluation on the
composed config; general (the reference's train-without-eval variant) is not built.  Uses Hydra when it is installed; otherwise `concepthash_amd.config` composes the same YAML
tree (hydra-core / omegaconf are absent from the target image).
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from concepthash_amd import config as cfglib

EVAL_KEYS = ("dataset", "data_dir", "work_dir", "eval_logdir", "R", "PRs", "use_last", "compute_mAP", "ternary_threshold",
             "dist_metric", "batch_size", "save_code", "sub_code_eval", "sub_code_eval_setting", "zero_mean_eval",
             "test_as_database")
# knobs of this implementation's evaluation loop (configs/val.yaml), overlaid the same way
LOOP_KEYS = ("eval_batch_min", "meter_stream", "tie_bracket", "tie_expected", "concept_eval", "hash_lookup_radii", "asymmetric_eval", "weight_bits", "text_eval",
             "prompt_prefix", "text_model", "ternary_eval", "ternary_margin", "dense_eval", "dense_metric", "rerank_eval", "rerank_metric",
             "rerank_shortlist", "itq_eval", "itq_blocks", "itq_iters", "reduce_eval", "reduce_bits", "reduce_method", "reduce_blocks",
             "reduce_iters")
# exp=search (configs/search.yaml, experiments/search.py): what it takes from the command line over the run's own config
SEARCH_KEYS = ("dataset", "data_dir", "work_dir", "search_logdir", "use_last", "batch_size", "zero_mean_eval", "query", "k", "concepts",
               "query_margin", "index", "rebuild_index", "save_attention", "rank", "index_margin", "weight_bits", "radius", "query_text", "query_text_file",
               "prompt_prefix", "text_model", "shortlist", "only_classes", "exclude_classes", "exclude_self", "same_class", "rotate",
               "rotate_blocks", "rotate_iters", "reduce", "reduce_bits", "reduce_blocks", "reduce_iters")


def _run_config(config, exp, keys):
    """<logdir>/config.yaml of a finished run with this invocation's `keys` (and the loop knobs) laid over it (reference main_v2.py:23-40)"""
    load_config = cfglib.load(os.path.join(config.logdir, "config.yaml"))
    for k in keys:
        load_config[k] = config[k]
    for k in LOOP_KEYS:
        if k in config:
            load_config[k] = config[k]
    load_config["logdir"] = config.logdir if os.path.isabs(str(config.logdir)) else f"{config.work_dir}/{config.logdir}"
    load_config["wandb"] = False
    load_config["exp"] = exp
    load_config["seed"] = config.get("seed", load_config.get("seed", 42))
    load_config["device"] = config.get("device", "cuda")
    return load_config


def run(config):
    from experiments.test_hashing import RetrievalEvaluation
    if config.exp == "general":
        raise NotImplementedError("exp='general' (train without evaluation, reference experiments/train_no_eval.py) is not built; "
                                  "use exp=hashing with eval_interval=0")
    if config.exp == "hashing":                  # reference main_v2.py:17-19
        from experiments.train_helper import RetrievalExperiment
        return RetrievalExperiment(config).main()
    if config.exp == "validation":
        load_config = _run_config(config, "validation", EVAL_KEYS)
        if load_config.get("tie_bracket"):      # the evaluator + the mAP bracket over tie orders
            from experiments.tie_bracket_eval import TieBracketEvaluation as RetrievalEvaluation
        if load_config.get("tie_expected"):     # ... + the mean over those orders (it extends the tie-bracket evaluator)
            from experiments.tie_expected_eval import TieExpectedEvaluation as RetrievalEvaluation
        if load_config.get("concept_eval"):     # ... + the per-concept table (it extends both)
            from experiments.concept_eval import ConceptEvaluation as RetrievalEvaluation
        if load_config.get("hash_lookup_radii") is not None:   # ... + hash lookup within Hamming radii (it extends both)
            from experiments.hash_lookup_eval import HashLookupEvaluation as RetrievalEvaluation
        if load_config.get("asymmetric_eval"):  # ... + every score once more under the asymmetric ranking (it extends all three)
            from experiments.asymmetric_eval import AsymmetricEvaluation as RetrievalEvaluation
        if load_config.get("text_eval"):        # ... + the class prompts as text queries against the database codes (it extends all four)
            from experiments.text_eval import TextEvaluation as RetrievalEvaluation
        if load_config.get("ternary_eval"):     # ... + every score once more under the ternary ranking (it extends all five)
            from experiments.ternary_eval import TernaryEvaluation as RetrievalEvaluation
        if load_config.get("dense_eval"):       # ... + every score once more under the ranking of the real-valued codes (it extends all six)
            from experiments.dense_eval import DenseEvaluation as RetrievalEvaluation
        if load_config.get("rerank_eval"):      # ... + every score once more on the two-stage list: Hamming shortlist, dense rerank (it extends all seven)
            from experiments.rerank_eval import RerankEvaluation as RetrievalEvaluation
        if load_config.get("itq_eval"):         # ... + the Hamming ranking once more after a rotation fitted to the database codes (it extends all eight)
            from experiments.itq_eval import ItqEvaluation as RetrievalEvaluation
        if load_config.get("reduce_eval"):      # ... + the Hamming ranking once more at reduce_bits bits, PCA(-ITQ) beside dropping bits (it extends all nine)
            from experiments.reduce_eval import ReduceEvaluation as RetrievalEvaluation
        experiment = RetrievalEvaluation(load_config)
    elif config.exp == "search":
        from experiments.search import SearchExperiment
        experiment = SearchExperiment(_run_config(config, "search", SEARCH_KEYS))
    elif config.exp in ("descriptor", "extract"):
        experiment = RetrievalEvaluation(config)
    else:
        raise ValueError(f'Unknown exp value: "{config.exp}"')
    return experiment.main()


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=True)
    ap.add_argument("--config-name", "-cn", default="train.yaml")
    ap.add_argument("--config-path", "-cp", default=os.path.join(ROOT, "configs"))
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    torch.multiprocessing.set_sharing_strategy("file_system")
    config = cfglib.compose(args.config_path, args.config_name, args.overrides, cwd=os.getcwd())
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:                                 # one process per GPU: data-parallel training, gallery-sharded retrieval
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        # nccl = RCCL over xGMI; CH_DIST_BACKEND=gloo only for rehearsing the multi-rank path with several ranks on ONE GPU
        backend = os.environ.get("CH_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    try:
        return run(config)
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
