"""`RetrievalEvaluation` that scores the two-stage list beside the Hamming one: config keys `rerank_eval: true`, `rerank_metric: cosine |
euclidean | dot`, `rerank_shortlist: <m>` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by the same call with `rank=<rerank_metric>, shortlist=<rerank_shortlist>` --
the list `exp=search rank=cosine shortlist=m` serves ("two-stage"): the first m database rows by Hamming
distance of the sign codes, ordered by the dense distance of the real-valued codes -- on the codes the evaluator hands over, i.e.
after `sub_code_eval`, `zero_mean_eval` and `test_as_database`.  `mAP_rerank{postfix}`, `recalls_rerank{postfix}`,
`precisions_rerank{postfix}`, `rerank_R{postfix}` (the effective R: -1 becomes the shortlist), `rerank_agreement{postfix}` ({k: the mean
share of the exhaustive dense top-k that the two-stage top-k holds}, for the k <= 128 of PRs), `rerank_metric` and `rerank_shortlist`
are added to the results and to `history.json` beside the call's own keys.  R and every k of PRs must be <= the shortlist (ValueError
from the metric).  Neither the metric nor the shortlist has a default.  It extends the dense evaluator, and through it the ternary,
text, asymmetric, hash-lookup, concept and tie-bracket ones, so their keys keep working beside it.
"""
from __future__ import annotations

import utils.hashing
from concepthash_amd.retrieval import DENSE_METRICS, RERANK_MAX, check_shortlist
from experiments.dense_eval import DenseEvaluation
from experiments.rank_rescoring import main_under_rank

KEYS = ("mAP_rerank", "recalls_rerank", "precisions_rerank")


def check_rerank_settings(metric, shortlist):
    """(`rerank_metric`, `rerank_shortlist`) of a `rerank_eval` run: one of DENSE_METRICS and an m in [1, 4096] (ValueError otherwise;
    None included -- neither has a default)"""
    if metric is None or str(metric) not in DENSE_METRICS:
        raise ValueError(f"rerank_eval: rerank_metric is required, one of {DENSE_METRICS} (there is no default), got {metric!r}")
    if shortlist is None:
        raise ValueError(f"rerank_eval: rerank_shortlist is required, an m in [1, {RERANK_MAX}] (there is no default)")
    return str(metric), check_shortlist(1, shortlist)[1]


class RerankEvaluation(DenseEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("rerank_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        metric, m = check_rerank_settings(cfg.get("rerank_metric"), cfg.get("rerank_shortlist"))
        left = []                           # utils.hashing.last_rerank of every repeated call, in the order of the calls

        def finish(res, calls):
            for (_, postfix, _), info in zip(calls, left):
                res["rerank_R" + postfix] = info["R"]
                res["rerank_agreement" + postfix] = {str(k): v for k, v in info["agreement"].items()}
            res["rerank_metric"], res["rerank_shortlist"] = metric, m

        return main_under_rank(self, super().main, "rerank_eval", dict(rank=metric, shortlist=m),
                               ("tie_bracket", "tie_expected", "radii", "rank", "weight_bits", "margin", "shortlist"),
                               f"{metric} over a Hamming shortlist of {m}", f"{metric}@{m}", KEYS,
                               on_call=lambda db_codes, test_codes: left.append(utils.hashing.last_rerank), finish=finish)
