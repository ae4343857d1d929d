"""`RetrievalEvaluation` with the per-concept table: config key `concept_eval: true` (configs/val.yaml).

`main_v2.py` runs this class instead of `experiments.test_hashing.RetrievalEvaluation` when the key is true (that module is left exactly
as it was; constructing its class directly does not read the key).  The code is concept-major -- concept c owns columns
[c nbit/Q, (c+1) nbit/Q) (models/arch/coop.py, csrc/head.hip) -- so every concept's sub-code is a column slice of the codes the evaluator
hands to `calculate_mAP`: already encoded and already post-processed (after `zero_mean_eval`).  Each such call is followed here by Q more
on the slices -- no encode -- and `mAP_concept{postfix}`, `recalls_concept{postfix}`, `precisions_concept{postfix}`, each a list of Q
entries (entry c = what `mAP` / `recalls` / `precisions` would be on concept c's columns), are added to the results and to
`history.json`.  It extends the tie-bracket and tie-expectation evaluators, so `tie_bracket: true` keeps working beside it (the bracket is
of the whole code) and `tie_expected: true` also records `mAP_concept_expected{postfix}`: every concept's mAP as the mean over the orders
of equal-distance rows -- a 16-bit sub-code has 17 distances, so this is where ties weigh most.
"""
from __future__ import annotations

import json
import os

import experiments.test_hashing as base
import utils.hashing
from experiments.test_hashing import _rows
from experiments.tie_expected_eval import TieExpectedEvaluation


class ConceptEvaluation(TieExpectedEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("concept_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        if cfg.get("sub_code_eval"):
            raise ValueError("concept_eval scores every concept's sub-code of the whole code; it cannot be combined with sub_code_eval")
        Q = int(cfg.model.ncontext)
        plain = utils.hashing.calculate_mAP
        calls = []                          # (the mAP object handed to the evaluator, the three per-concept lists) per calculate_mAP call

        def with_concepts(db_codes, db_labels, test_codes, test_labels, R, **k):
            nbit = int(db_codes.shape[1])
            if nbit % Q:
                raise ValueError(f"concept_eval: {nbit} code columns are not a multiple of ncontext = {Q}")
            sb = nbit // Q
            per = {key: v for key, v in k.items() if key != "tie_bracket"}     # the bracket, when asked for, is of the whole code
            mAPs, recalls, precisions, expected = [], [], [], []
            for c in range(Q):
                cut = lambda t, a=c * sb, b=(c + 1) * sb: t[:, a:b]
                m, r, p = plain(_rows(db_codes, cut), db_labels, _rows(test_codes, cut), test_labels, R, **per)
                mAPs.append(m), recalls.append(r), precisions.append(p)
                if per.get("tie_expected"):          # the tie-expectation evaluator asks for it: each sub-code's own expectation
                    expected.append(utils.hashing.last_tie_expected["mAP_expected"])
                print(f"concept {c} (bits {c * sb}-{(c + 1) * sb - 1}): mAP@{R}: " +
                      (", ".join(f"{x:.4f}" for x in m) if isinstance(m, list) else f"{m:.4f}") +
                      "; " + " ".join(f"P@{kk}: {x:.4f}" for kk, x in zip(k.get("PRs") or [], p)))
            out = plain(db_codes, db_labels, test_codes, test_labels, R, **k)   # last: a tie bracket it leaves behind is the whole code's
            calls.append((out[0], (mAPs, recalls, precisions), expected))
            return out
        # The evaluator calls the name `calculate_mAP` of its own module; the tie-bracket evaluator rebinds that name for its run and calls
        # `utils.hashing.calculate_mAP` from there.  So the name wrapped for the length of this run is the one that will be called.
        owner = utils.hashing if cfg.get("tie_bracket") else base
        owner.calculate_mAP = with_concepts
        try:
            res = super().main()
        finally:
            owner.calculate_mAP = plain
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, (mAPs, recalls, precisions), expected in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"concept_eval: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            res["mAP_concept" + postfix], res["recalls_concept" + postfix], res["precisions_concept" + postfix] = mAPs, recalls, precisions
            if expected:
                res["mAP_concept_expected" + postfix] = expected
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
