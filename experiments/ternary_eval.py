"""`RetrievalEvaluation` that scores the ternary ranking beside the Hamming one: config keys `ternary_eval: true`,
`ternary_margin: <m>` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by the same call with `rank="ternary", margin=m` -- the ranking `exp=search
rank=ternary` serves: both code sets become ternary codes, sign(x) where |x| > m and 0 otherwise, ranked by
K = nbit - t_q . t_g -- on the codes the evaluator hands over, i.e. after `sub_code_eval`, `zero_mean_eval` and `test_as_database`.
`mAP_ternary{postfix}`, `recalls_ternary{postfix}`, `precisions_ternary{postfix}`, `ternary_margin` and `ternary_zero_share` (the share
of zeros among the ternary database and query codes of the last such call, [database, queries]) are added to the results and to
`history.json` beside the call's own keys.  The margin has no default: the scale of the codes belongs to the run.  It extends the text,
asymmetric, hash-lookup, concept and tie-bracket evaluators, so their keys keep working beside it (the bracket, the radii, the
per-concept table, the asymmetric triple and the text queries stay what they were: calls under another rank, the concepts' column
slices and the text queries' call are passed through).
"""
from __future__ import annotations

import torch

from concepthash_amd.retrieval import check_margin
from experiments.rank_rescoring import main_under_rank
from experiments.text_eval import TextEvaluation

KEYS = ("mAP_ternary", "recalls_ternary", "precisions_ternary")


def zero_share(codes, margin: float) -> float:
    """share of the entries of real codes that the margin turns into ternary 0 (|x| <= margin, or NaN)"""
    x = torch.as_tensor(codes)
    return 1.0 - float((x.abs() > margin).double().mean()) if x.numel() else 0.0


class TernaryEvaluation(TextEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("ternary_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        margin = check_margin(cfg.get("ternary_margin"), "ternary_eval: ternary_margin")
        shares = []

        def on_call(db_codes, test_codes):
            shares[:] = [zero_share(db_codes, margin), zero_share(test_codes, margin)]

        return main_under_rank(self, super().main, "ternary_eval", dict(rank="ternary", margin=margin),
                               ("tie_bracket", "tie_expected", "radii", "rank", "weight_bits"), f"ternary, margin {margin:g}", "ternary", KEYS, on_call,
                               lambda res, calls: res.update(ternary_margin=margin, ternary_zero_share=list(shares)))
