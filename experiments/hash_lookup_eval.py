"""`RetrievalEvaluation` with hash lookup within Hamming radii: config key `hash_lookup_radii: [0, 2]`
(configs/val.yaml).

`main_v2.py` runs this class when the key is a list (experiments.test_hashing is left exactly as it was).  Every `calculate_mAP` call of
the evaluator then also asks for the lookup statistics at those radii -- they come from the histogram the call builds anyway -- and
`precisions_radius{postfix}`, `recalls_radius{postfix}`, `retrieved_radius{postfix}`, `empty_radius{postfix}` (lists, one entry per
radius) are added to the results and to `history.json` beside the call's own keys.  It extends the concept and tie-bracket evaluators, so
both keys keep working beside it.
"""
from __future__ import annotations

import json
import os

import experiments.test_hashing as base
import utils.hashing
from experiments.concept_eval import ConceptEvaluation

KEYS = ("precisions_radius", "recalls_radius", "retrieved_radius", "empty_radius")


class HashLookupEvaluation(ConceptEvaluation):
    def main(self):
        cfg = self.config
        radii = cfg.get("hash_lookup_radii")
        if radii is None or not cfg.get("compute_mAP") or cfg.exp == "extract":
            return super().main()
        radii = [int(r) for r in radii]
        plain_metric, plain_name = utils.hashing.calculate_mAP, base.calculate_mAP
        calls = []                          # (the mAP object of a whole-code call, its lookup statistics)
        # Under concept_eval every call of the evaluator reaches this wrapper as Q calls on the concepts' column slices followed by the call
        # on the whole code (experiments/concept_eval.py).  Only the whole-code call takes the radii; the slices pass through untouched.
        Q = int(cfg.model.ncontext) if cfg.get("concept_eval") else 0
        slices = []                         # widths of the per-concept calls since the last whole-code call

        def with_lookup(db_codes, db_labels, test_codes, test_labels, R, **k):
            width = int(db_codes.shape[1])
            if len(slices) < Q:
                slices.append(width)
                return plain_metric(db_codes, db_labels, test_codes, test_labels, R, **k)
            if any(w * Q != width for w in slices):
                raise RuntimeError(f"hash lookup: expected {Q} per-concept calls of {width // max(Q, 1)} columns in front of a call on {width} "
                                   f"columns, saw widths {slices}")
            slices.clear()
            out = plain_metric(db_codes, db_labels, test_codes, test_labels, R, radii=radii, **k)
            look = utils.hashing.last_hash_lookup
            if look is None:
                raise RuntimeError("hash lookup: calculate_mAP(radii=...) left no utils.hashing.last_hash_lookup")
            calls.append((out[0], look))
            return out
        # The innermost name: the evaluator calls `calculate_mAP` of its own module; the tie-bracket and concept evaluators rebind that name
        # (or utils.hashing's) for their run and end up in `utils.hashing.calculate_mAP`.  Both names are wrapped for the length of this run.
        utils.hashing.calculate_mAP = base.calculate_mAP = with_lookup
        try:
            res = super().main()
        finally:
            utils.hashing.calculate_mAP, base.calculate_mAP = plain_metric, plain_name
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, look in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"hash lookup: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            for key in KEYS:
                res[key + postfix] = look[key]
            print(f"hash lookup{postfix}: " + "  ".join(f"H<={r}: P {p:.4f} R {rc:.4f} rows {n:.1f} empty {e:.3f}" for r, p, rc, n, e in
                                                       zip(radii, *(look[key] for key in KEYS))))
        res["hash_lookup_radii"] = radii
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
