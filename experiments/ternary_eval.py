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

import json
import os

import torch

import experiments.test_hashing as base
import utils.hashing
from concepthash_amd.retrieval import check_margin
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
        metric, name = utils.hashing.calculate_mAP, base.calculate_mAP
        calls = []                          # (the mAP object of a whole-code call, its triple under the ternary ranking)
        shares = []
        # Under concept_eval the metric is reached Q times on the concepts' column slices in front of the call on the whole code
        # (experiments/concept_eval.py); only the whole-code call is repeated under the ternary ranking.
        Q = int(cfg.model.ncontext) if cfg.get("concept_eval") else 0
        slices = []                         # widths of the per-concept calls since the last whole-code call
        text_call = []                      # non-empty while the text evaluator scores its prompts: that call is not the evaluator's

        def with_ternary(db_codes, db_labels, test_codes, test_labels, R, **k):
            out = metric(db_codes, db_labels, test_codes, test_labels, R, **k)
            if k.get("rank", "hamming") != "hamming" or text_call:
                return out
            width = int(db_codes.shape[1])
            if len(slices) < Q:
                slices.append(width)
                return out
            if any(w * Q != width for w in slices):
                raise RuntimeError(f"ternary_eval: expected {Q} per-concept calls of {width // max(Q, 1)} columns in front of a call on "
                                   f"{width} columns, saw widths {slices}")
            slices.clear()
            # the bracket and the lookup the Hamming call left behind are read by the evaluators around this one after it returns
            left = utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup
            own = {key: v for key, v in k.items() if key not in ("tie_bracket", "radii", "rank", "weight_bits")}
            tern = metric(db_codes, db_labels, test_codes, test_labels, R, rank="ternary", margin=margin, **own)
            utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup = left
            calls.append((out[0], tern))
            shares[:] = [zero_share(db_codes, margin), zero_share(test_codes, margin)]
            many = isinstance(tern[0], list)
            for r_, m in (zip(R, tern[0]) if many else [(R, tern[0])]):
                print(f"mAP@{r_} (ternary, margin {margin:g}): {m:.4f}")
            for kk, r, p in zip(k.get("PRs") or [], tern[1], tern[2]):
                print(f"P@{kk} (ternary): {p:.4f}; R@{kk} (ternary): {r:.4f}")
            return out
        # This wrapper stands where the metric itself stood, under both names it is reached by: every evaluator this one extends rebinds
        # one of the two names for its run on top of it, so it is the last stop in front of `utils.hashing.calculate_mAP`.
        utils.hashing.calculate_mAP = base.calculate_mAP = with_ternary
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
        for mAP, tern in calls:
            keys = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
            if len(keys) != 1:
                raise RuntimeError(f"ternary_eval: a calculate_mAP result is stored under {keys} in the results, expected one key")
            postfix = keys[0][len("mAP"):]
            for key, v in zip(KEYS, tern):
                res[key + postfix] = v
        res["ternary_margin"] = margin
        res["ternary_zero_share"] = list(shares)
        if self.rank == 0:
            with open(os.path.join(self.eval_logdir, "history.json"), "w") as f:
                json.dump(res, f)
        self.results = res
        return res
