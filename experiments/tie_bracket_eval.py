"""`RetrievalEvaluation` with the tie bracket: config key `tie_bracket: true`.

`main_v2.py` runs this class instead of `experiments.test_hashing.RetrievalEvaluation` when the key is true (that module is left
exactly as it was; constructing its class directly does not read the key).  Every `calculate_mAP` call the evaluator makes then asks
for the bracket as well: the line `mAP@R: 0.8123  [0.8101, 0.8150] over tie orders` is printed per R as the call returns, i.e. directly
above the evaluator's own `mAP@R` / `P@k` lines of that output, and `mAP_tie_low{postfix}` / `mAP_tie_high{postfix}` -- the smallest /
largest mAP over every order of the database rows at equal Hamming distance -- are added to the results and to `history.json`.
"""
from __future__ import annotations

import json
import os

import experiments.test_hashing as base
import utils.hashing


class TieBracketEvaluation(base.RetrievalEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("tie_bracket") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        calls = []                          # (the mAP object handed to the evaluator, its bracket) per calculate_mAP call

        def with_bracket(db_codes, db_labels, test_codes, test_labels, R, **k):
            out = utils.hashing.calculate_mAP(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=True, **k)
            br = utils.hashing.last_tie_bracket
            calls.append((out[0], br))
            many = isinstance(out[0], list)
            for r_, m, lo, hi in (zip(R, out[0], br["mAP_low"], br["mAP_high"]) if many else [(R, out[0], br["mAP_low"], br["mAP_high"])]):
                print(f"mAP@{r_}: {m:.4f}  [{lo:.4f}, {hi:.4f}] over tie orders")
            return out
        # the evaluator calls the name `calculate_mAP` of its own module: it is rebound for the length of this run only
        plain = base.calculate_mAP
        base.calculate_mAP = with_bracket
        try:
            res = super().main()
        finally:
            base.calculate_mAP = plain
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, br in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"tie bracket: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            res["mAP_tie_low" + postfix], res["mAP_tie_high" + postfix] = br["mAP_low"], br["mAP_high"]
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
