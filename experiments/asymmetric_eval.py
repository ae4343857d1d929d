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

import json
import os

import experiments.test_hashing as base
import utils.hashing
from experiments.hash_lookup_eval import HashLookupEvaluation

KEYS = ("mAP_asymmetric", "recalls_asymmetric", "precisions_asymmetric")


class AsymmetricEvaluation(HashLookupEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("asymmetric_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        bits = int(cfg.get("weight_bits", 8))
        metric, name = utils.hashing.calculate_mAP, base.calculate_mAP
        calls = []                          # (the mAP object of a whole-code call, its triple under the asymmetric ranking)
        # Under concept_eval the metric is reached Q times on the concepts' column slices in front of the call on the whole code
        # (experiments/concept_eval.py); only the whole-code call is repeated under the asymmetric ranking.
        Q = int(cfg.model.ncontext) if cfg.get("concept_eval") else 0
        slices = []                         # widths of the per-concept calls since the last whole-code call

        def with_asymmetric(db_codes, db_labels, test_codes, test_labels, R, **k):
            out = metric(db_codes, db_labels, test_codes, test_labels, R, **k)
            width = int(db_codes.shape[1])
            if len(slices) < Q:
                slices.append(width)
                return out
            if any(w * Q != width for w in slices):
                raise RuntimeError(f"asymmetric_eval: expected {Q} per-concept calls of {width // max(Q, 1)} columns in front of a call on "
                                   f"{width} columns, saw widths {slices}")
            slices.clear()
            # the bracket and the lookup the Hamming call left behind are read by the evaluators around this one after it returns
            left = utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup
            own = {key: v for key, v in k.items() if key not in ("tie_bracket", "radii")}
            asym = metric(db_codes, db_labels, test_codes, test_labels, R, rank="asymmetric", weight_bits=bits, **own)
            utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup = left
            calls.append((out[0], asym))
            many = isinstance(asym[0], list)
            for r_, m in (zip(R, asym[0]) if many else [(R, asym[0])]):
                print(f"mAP@{r_} (asymmetric, {bits}-bit weights): {m:.4f}")
            for kk, r, p in zip(k.get("PRs") or [], asym[1], asym[2]):
                print(f"P@{kk} (asymmetric): {p:.4f}; R@{kk} (asymmetric): {r:.4f}")
            return out
        # This wrapper stands where the metric itself stood, under both names it is reached by: the evaluator calls `calculate_mAP` of its
        # own module, and the evaluators this one extends rebind that name (or utils.hashing's) for their run and end up in
        # `utils.hashing.calculate_mAP`.
        utils.hashing.calculate_mAP = base.calculate_mAP = with_asymmetric
        try:
            res = super().main()
        finally:
            utils.hashing.calculate_mAP, base.calculate_mAP = metric, name
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, asym in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"asymmetric_eval: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            for key, v in zip(KEYS, asym):
                res[key + postfix] = v
        res["weight_bits"] = bits
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
