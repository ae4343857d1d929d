"""One definition of "score every whole-code `calculate_mAP` call of the evaluator again under another rank", for the evaluators that
do so: `AsymmetricEvaluation`, `TernaryEvaluation` and `DenseEvaluation` (experiments/asymmetric_eval.py, ternary_eval.py,
dense_eval.py).  Each of them states its config key and argument check, the keyword arguments of the repeated call, its labels, its
result keys and its extra results; the rest is here.
"""
from __future__ import annotations

import json
import os

import experiments.test_hashing as base
import utils.hashing


def main_under_rank(ev, run, who: str, again: dict, drop, label: str, short: str, keys, on_call=None, finish=None, recode=None, also=()) -> dict:
    """`run()` -- the main() of the class that the calling class extends -- with every whole-code `calculate_mAP` call of the evaluator
    followed by the same call with the keyword arguments `again` (rank=..., and what goes with it) in place of those named in `drop`,
    on the codes the evaluator hands over.  The triple of a repeated call is printed under `label` (mAP) and `short` (P@k, R@k) and stored
    under `keys` + the postfix of the call's own "mAP" key; `on_call(db_codes, test_codes)` sees every repeated call's codes;
    `finish(res, calls)`, calls = [(the call's own mAP, postfix, its triple under the rank)], adds the class's extra results before
    `history.json` is written again.  `who` (the config key) opens the error messages.  `recode(db_codes, db_labels, test_codes,
    test_labels) -> (db_codes, test_codes)`, where given, makes the codes of the repeated call from the evaluator's (the learned rotation).
    `also`: further repeated calls of the same kind, each (its keys, its recode, its label) -- the reduction's truncation baseline; their
    triples are stored under their keys + the postfix, printed under their label, and not handed to `finish`.
    Passed through, scored once: a call under another rank (an evaluator further out repeating its own), the concepts' column slices
    -- under concept_eval the metric is reached Q times on them in front of the call on the whole code (experiments/concept_eval.py) --
    and the text evaluator's call on its prompts."""
    cfg = ev.config
    metric, name = utils.hashing.calculate_mAP, base.calculate_mAP
    calls = []                          # (the mAP object of a whole-code call, its triple under the rank)
    Q = int(cfg.model.ncontext) if cfg.get("concept_eval") else 0
    slices = []                         # widths of the per-concept calls since the last whole-code call
    text_call = []                      # non-empty while the text evaluator scores its prompts: that call is not the evaluator's

    def with_rank(db_codes, db_labels, test_codes, test_labels, R, **k):
        out = metric(db_codes, db_labels, test_codes, test_labels, R, **k)
        if k.get("rank", "hamming") != "hamming" or text_call:
            return out
        width = int(db_codes.shape[1])
        if len(slices) < Q:
            slices.append(width)
            return out
        if any(w * Q != width for w in slices):
            raise RuntimeError(f"{who}: expected {Q} per-concept calls of {width // max(Q, 1)} columns in front of a call on "
                               f"{width} columns, saw widths {slices}")
        slices.clear()
        # the bracket and the lookup the Hamming call left behind are read by the evaluators around this one after it returns
        left = utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup, utils.hashing.last_tie_expected
        db_again, test_again = (db_codes, test_codes) if recode is None else recode(db_codes, db_labels, test_codes, test_labels)
        other = metric(db_again, db_labels, test_again, test_labels, R, **again, **{key: v for key, v in k.items() if key not in drop})
        utils.hashing.last_tie_bracket, utils.hashing.last_hash_lookup, utils.hashing.last_tie_expected = left
        more = []
        for _, rc, _ in also:
            db_more, test_more = rc(db_codes, db_labels, test_codes, test_labels)
            more.append(metric(db_more, db_labels, test_more, test_labels, R, **again, **{key: v for key, v in k.items() if key not in drop}))
        calls.append((out[0], other, more))
        if on_call is not None:
            on_call(db_codes, test_codes)
        many = isinstance(other[0], list)
        for r_, m in (zip(R, other[0]) if many else [(R, other[0])]):
            print(f"mAP@{r_} ({label}): {m:.4f}")
        for kk, r, p in zip(k.get("PRs") or [], other[1], other[2]):
            print(f"P@{kk} ({short}): {p:.4f}; R@{kk} ({short}): {r:.4f}")
        for (_, _, label_more), triple in zip(also, more):
            for r_, m in (zip(R, triple[0]) if many else [(R, triple[0])]):
                print(f"mAP@{r_} ({label_more}): {m:.4f}")
        return out
    # This wrapper stands where the metric itself stood, under both names it is reached by: the evaluator calls `calculate_mAP` of its
    # own module, and the evaluators the calling class extends rebind that name (or utils.hashing's) for their run on top of it and end
    # up in `utils.hashing.calculate_mAP`.
    utils.hashing.calculate_mAP = base.calculate_mAP = with_rank
    phase = getattr(ev, "_phase", None)
    if phase is not None:
        def marking(pname, fn, *a, **k):
            if pname != "retrieval_text":
                return phase(pname, fn, *a, **k)
            text_call.append(pname)
            try:
                return phase(pname, fn, *a, **k)
            finally:
                text_call.clear()
        ev._phase = marking
    try:
        res = run()
    finally:
        utils.hashing.calculate_mAP, base.calculate_mAP = metric, name
        if phase is not None:
            ev._phase = phase
    # the evaluator stored each call's mAP object under "mAP" + postfix: find it by identity, not by position or key order
    stored = []
    for mAP, other, more in calls:
        found = [k for k, v in res.items() if v is mAP and k.startswith("mAP")]
        if len(found) != 1:
            raise RuntimeError(f"{who}: a calculate_mAP result is stored under {found} in the results, expected one key")
        postfix = found[0][len("mAP"):]
        for key, v in zip(keys, other):
            res[key + postfix] = v
        for (keys_more, _, _), triple in zip(also, more):
            for key, v in zip(keys_more, triple):
                res[key + postfix] = v
        stored.append((mAP, postfix, other))
    if finish is not None:
        finish(res, stored)
    if ev.rank == 0:
        with open(os.path.join(ev.eval_logdir, "history.json"), "w") as f:
            json.dump(res, f)
    ev.results = res
    return res
