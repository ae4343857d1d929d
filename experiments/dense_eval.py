"""`RetrievalEvaluation` that scores the ranking of the real-valued codes beside the Hamming one: config keys `dense_eval: true`,
`dense_metric: cosine | euclidean | dot` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by the same call with `rank=<dense_metric>` -- the ranking `exp=search
rank=cosine` serves: neither code set is binarised -- on the codes the evaluator hands over, i.e. after
`sub_code_eval`, `zero_mean_eval` and `test_as_database`.  `mAP_dense{postfix}`, `recalls_dense{postfix}`, `precisions_dense{postfix}`,
`dense_metric` and `quantisation_gap{postfix}` = mAP_dense - mAP, what binarising the codes costs the run (a list where mAP is a list),
are added to the results and to `history.json` beside the call's own keys.  The metric has no default.  It extends the ternary, text,
asymmetric, hash-lookup, concept and tie-bracket evaluators, so their keys keep working beside it: calls under another rank, the
concepts' column slices and the text queries' call are passed through.
"""
from __future__ import annotations

from concepthash_amd.retrieval import DENSE_METRICS
from experiments.rank_rescoring import main_under_rank
from experiments.ternary_eval import TernaryEvaluation

KEYS = ("mAP_dense", "recalls_dense", "precisions_dense")


def check_dense_metric(metric) -> str:
    """`dense_metric` of a `dense_eval` run: one of DENSE_METRICS (ValueError otherwise; None included -- there is no default)"""
    if metric is None:
        raise ValueError(f"dense_eval: dense_metric is required, one of {DENSE_METRICS} (there is no default)")
    if str(metric) not in DENSE_METRICS:
        raise ValueError(f"dense_eval: dense_metric must be one of {DENSE_METRICS}, got {metric!r}")
    return str(metric)


class DenseEvaluation(TernaryEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("dense_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        dense = check_dense_metric(cfg.get("dense_metric"))

        def finish(res, calls):
            for mAP, postfix, real in calls:
                res["quantisation_gap" + postfix] = [d - h for d, h in zip(real[0], mAP)] if isinstance(mAP, list) else real[0] - mAP
            res["dense_metric"] = dense

        return main_under_rank(self, super().main, "dense_eval", dict(rank=dense), ("tie_bracket", "tie_expected", "radii", "rank", "weight_bits", "margin"),
                               f"{dense}, real-valued codes", dense, KEYS, finish=finish)
