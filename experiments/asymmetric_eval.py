"""`RetrievalEvaluation` that scores the asymmetric (weighted) ranking beside the Hamming one: config keys `asymmetric_eval: true`,
`weight_bits: 8` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by the same call with `rank="asymmetric"` -- the ranking `exp=search
rank=asymmetric` serves: the query codes keep their real values, the database is sign-packed as ever -- on the
codes the evaluator hands over, i.e. after `sub_code_eval`, `zero_mean_eval` and `test_as_database`.  `mAP_asymmetric{postfix}`,
`recalls_asymmetric{postfix}`, `precisions_asymmetric{postfix}` and `weight_bits` are added to the results and to `history.json` beside
the call's own keys.  It extends the hash-lookup, concept and tie-bracket evaluators, so their keys keep working beside it (the bracket,
the radii and the per-concept table stay Hamming statistics).
"""
from __future__ import annotations

from experiments.hash_lookup_eval import HashLookupEvaluation
from experiments.rank_rescoring import main_under_rank

KEYS = ("mAP_asymmetric", "recalls_asymmetric", "precisions_asymmetric")


class AsymmetricEvaluation(HashLookupEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("asymmetric_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        bits = int(cfg.get("weight_bits", 8))
        # The shared body passes a call under another rank and the text evaluator's call through.  Neither reaches this evaluator -- no
        # caller below it passes a `rank`, and the text evaluator extends it, so its call is made after this main() has returned -- so
        # the guard changes nothing here.
        return main_under_rank(self, super().main, "asymmetric_eval", dict(rank="asymmetric", weight_bits=bits), ("tie_bracket", "tie_expected", "radii"),
                               f"asymmetric, {bits}-bit weights", "asymmetric", KEYS,
                               finish=lambda res, calls: res.update(weight_bits=bits))
