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

import json
import os

import experiments.test_hashing as base
import utils.hashing
from concepthash_amd.retrieval import DENSE_METRICS
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
        metric, name = utils.hashing.calculate_mAP, base.calculate_mAP
        calls = []                          # (the mAP object of a whole-code call, its triple under the dense ranking)
        # Under concept_eval the metric is reached Q times on the concepts' column slices in front of the call on the whole code
        # (experiments/concept_eval.py); only the whole-code call is repeated under the dense ranking.
        Q = int(cfg.model.ncontext) if cfg.get("concept_eval") else 0
        slices = []                         # widths of the per-concept calls since the last whole-code call
        text_call = []                      # non-empty while the text evaluator scores its prompts: that call is not the evaluator's

        def with_dense(db_codes, db_labels, test_codes, test_labels, R, **k):
            out = metric(db_codes, db_labels, test_codes, test_labels, R, **k)
            if k.get("rank", "hamming") != "hamming" or text_call:
                return out
            width = int(db_codes.shape[1])
            if len(slices) < Q:
                slices.append(width)
                return out
            if any(w * Q != width for w in slices):
                raise RuntimeError(f"dense_eval: expected {Q} per-concept calls of {width // max(Q, 1)} columns in front of a call on "
                                   f"{width} columns, saw widths {slices}")
            slices.clear()
            # the bracket and the lookup the Hamming call left behind are read by the evaluators around this one after it returns
            left = utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup
            own = {key: v for key, v in k.items() if key not in ("tie_bracket", "radii", "rank", "weight_bits", "margin")}
            real = metric(db_codes, db_labels, test_codes, test_labels, R, rank=dense, **own)
            utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup = left
            calls.append((out[0], real))
            many = isinstance(real[0], list)
            for r_, m in (zip(R, real[0]) if many else [(R, real[0])]):
                print(f"mAP@{r_} ({dense}, real-valued codes): {m:.4f}")
            for kk, r, p in zip(k.get("PRs") or [], real[1], real[2]):
                print(f"P@{kk} ({dense}): {p:.4f}; R@{kk} ({dense}): {r:.4f}")
            return out
        # This wrapper stands where the metric itself stood, under both names it is reached by: every evaluator this one extends rebinds
        # one of the two names for its run on top of it, so it is the last stop in front of `utils.hashing.calculate_mAP`.
        utils.hashing.calculate_mAP = base.calculate_mAP = with_dense
        phase = getattr(self, "_phase", None)
        if phase is not None:
            def marking(pname, fn, *a, **k):
                if pname != "retrieval_text":
                    return phase(pname, fn, *a, **k)
                text_call.append(pname)
                try:
                    return phase(pname, fn, *a, **k)
                finally:
                    text_call.clear()
            self._phase = marking
        try:
            res = super().main()
        finally:
            utils.hashing.calculate_mAP, base.calculate_mAP = metric, name
            if phase is not None:
                self._phase = phase
        # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
        for mAP, real in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"dense_eval: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            for key, v in zip(KEYS, real):
                res[key + postfix] = v
            res["quantisation_gap" + postfix] = [d - h for d, h in zip(real[0], mAP)] if isinstance(mAP, list) else real[0] - mAP
        res["dense_metric"] = dense
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
