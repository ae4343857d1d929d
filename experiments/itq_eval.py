"""`RetrievalEvaluation` that scores the Hamming ranking once more after a learned rotation: config keys `itq_eval: true`,
`itq_blocks: <int, default the model's ncontext>`, `itq_iters: 50` (configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by the same Hamming call on rotated codes: a block-diagonal rotation is fitted
by iterative quantisation (`retrieval.fit_rotation`; DESIGN.md section 2.0, "learned rotation") to the DATABASE codes the evaluator
hands over -- after `sub_code_eval`, `zero_mean_eval` and `test_as_database` -- and applied to both code sets, which is what
`exp=search rotate=itq` serves.  `mAP_itq{postfix}`, `recalls_itq{postfix}`, `precisions_itq{postfix}`, `itq_iters_run{postfix}`,
`quantisation_error{postfix}` and `quantisation_error_itq{postfix}` (mean_i 1 - |z_i|_1 / (sqrt(n) |z_i|_2) of the database codes
before and after), `itq_gain{postfix}` = mAP_itq - mAP (a list where mAP is a list) and `itq_blocks` are added to the results and to
`history.json` beside the call's own keys.  Single process only (NotImplementedError for RowShards or more than one rank, as the
other re-scored rankings).  It extends the rerank evaluator, and through it every other one, so their keys keep working beside it.
"""
from __future__ import annotations

import torch

import utils.hashing
from concepthash_amd import retrieval as rt
from experiments.rank_rescoring import main_under_rank
from experiments.rerank_eval import RerankEvaluation

KEYS = ("mAP_itq", "recalls_itq", "precisions_itq")


def check_itq_settings(blocks, iters, ncontext: int):
    """(`itq_blocks`, `itq_iters`) of an `itq_eval` run: ints >= 1, blocks defaulting to the model's ncontext (ValueError otherwise)"""
    blocks = int(ncontext) if blocks is None else blocks
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 1:
        raise ValueError(f"itq_eval: itq_blocks must be an int >= 1, got {blocks!r}")
    iters = 50 if iters is None else iters
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"itq_eval: itq_iters must be an int >= 1, got {iters!r}")
    return blocks, iters


def rotated_pair(db_codes, test_codes, blocks: int, iters: int):
    """Fit on the database codes, rotate both sets -> (db, test, the fit).  `blocks` not dividing the evaluated width: ValueError."""
    width = int(db_codes.shape[1])
    if width % blocks:
        raise ValueError(f"itq_eval: itq_blocks = {blocks} does not divide the evaluated code width {width}")
    dev = utils.hashing._device()
    db = torch.as_tensor(db_codes).to(dev, torch.float32).contiguous()
    test = torch.as_tensor(test_codes).to(dev, torch.float32).contiguous()
    fit = rt.fit_rotation(db, blocks, iters)
    return rt.rotate_codes(db, fit["R"], blocks), rt.rotate_codes(test, fit["R"], blocks), fit


class ItqEvaluation(RerankEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("itq_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        blocks, iters = check_itq_settings(cfg.get("itq_blocks"), cfg.get("itq_iters"), int(cfg.model.ncontext))
        fits = []                           # the fit of every repeated call, in the order of the calls

        def recode(db_codes, db_labels, test_codes, test_labels):
            utils.hashing._single_process("hamming after itq_eval", db_codes, db_labels, test_codes, test_labels)
            db, test, fit = rotated_pair(db_codes, test_codes, blocks, iters)
            fits.append(fit)
            return db, test

        def finish(res, calls):
            for (mAP, postfix, rot), fit in zip(calls, fits):
                res["itq_iters_run" + postfix] = fit["iters_run"]
                res["quantisation_error" + postfix], res["quantisation_error_itq" + postfix] = fit["qerr_before"], fit["qerr_after"]
                res["itq_gain" + postfix] = [r - h for r, h in zip(rot[0], mAP)] if isinstance(mAP, list) else rot[0] - mAP
            res["itq_blocks"] = blocks

        return main_under_rank(self, super().main, "itq_eval", {}, ("tie_bracket", "tie_expected", "radii", "rank", "weight_bits", "margin", "shortlist"),
                               f"Hamming, after ITQ in {blocks} blocks", "itq", KEYS, finish=finish, recode=recode)
