"""`RetrievalEvaluation` with the tie expectation: config key `tie_expected: true`.

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every Hamming `calculate_mAP`
call the evaluator makes then also asks for the mean of every statistic over the orders of equal-distance database rows: the line
`mAP@R: 0.8123  expected 0.8119 over tie orders` is printed per R as the call returns, and `mAP_expected{postfix}`,
`precisions_expected{postfix}`, `recalls_expected{postfix}` are added to the results and to `history.json`.  It extends the tie-bracket
evaluator, so both keys work together or apart; the concept evaluator extends this one and records `mAP_concept_expected` beside it.
"""
from __future__ import annotations

import json
import os

import experiments.test_hashing as base
import utils.hashing
from experiments.tie_bracket_eval import TieBracketEvaluation

KEYS = ("mAP_expected", "precisions_expected", "recalls_expected")


class TieExpectedEvaluation(TieBracketEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("tie_expected") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        calls = []                          # (the mAP object handed to the evaluator, its expectation) per calculate_mAP call
        # The evaluator calls the name `calculate_mAP` of its own module; the tie-bracket evaluator rebinds that name for its run and calls
        # `utils.hashing.calculate_mAP` from there.  So the name wrapped for the length of this run is the one that will be called (the
        # concept evaluator, which runs around this one, has made the same choice: its wrapper is what `inner` finds there).
        owner = utils.hashing if cfg.get("tie_bracket") else base
        inner = owner.calculate_mAP

        def with_expected(db_codes, db_labels, test_codes, test_labels, R, **k):
            if k.get("rank", "hamming") != "hamming":       # the expectation is defined on Hamming distances
                return inner(db_codes, db_labels, test_codes, test_labels, R, **k)
            out = inner(db_codes, db_labels, test_codes, test_labels, R, tie_expected=True, **k)
            ex = utils.hashing.last_tie_expected
            if ex is None:
                raise RuntimeError("tie expectation: calculate_mAP(tie_expected=True) left no utils.hashing.last_tie_expected")
            calls.append((out[0], ex))
            many = isinstance(out[0], list)
            for r_, m, e in (zip(R, out[0], ex["mAP_expected"]) if many else [(R, out[0], ex["mAP_expected"])]):
                print(f"mAP@{r_}: {m:.4f}  expected {e:.4f} over tie orders")
            return out
        owner.calculate_mAP = with_expected
        try:
            res = super().main()
        finally:
            owner.calculate_mAP = inner
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, ex in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"tie expectation: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            for key in KEYS:
                res[key + postfix] = ex[key]
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
