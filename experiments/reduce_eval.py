"""`RetrievalEvaluation` that scores the Hamming ranking once more at a shorter code length: config keys `reduce_eval: true`,
`reduce_bits: <m>` (required), `reduce_method: pca-itq | pca`, `reduce_blocks: <int, default the model's ncontext>`, `reduce_iters: 50`
(configs/val.yaml).

`main_v2.py` runs this class when the key is true (experiments.test_hashing is left exactly as it was).  Every whole-code
`calculate_mAP` call of the evaluator is then followed by two Hamming calls at `reduce_bits` bits: on codes reduced by a block-wise
PCA(-ITQ) (`retrieval.fit_reduction`; DESIGN.md section 2.0, "reduction") fitted to the DATABASE codes the evaluator hands over -- after
`zero_mean_eval`, `sub_code_eval` and `test_as_database` -- and applied to both code sets through ONE chain
(`retrieval.project_codes`), which is what `exp=search reduce=...` serves; and on the first `reduce_bits / reduce_blocks` columns of
every block of the codes as they are -- what dropping bits gives.  `mAP_reduce{postfix}`, `recalls_reduce{postfix}`,
`precisions_reduce{postfix}`, `reduce_iters_run{postfix}`, `reduce_explained{postfix}` (the kept eigenvalues' share of the variance),
`quantisation_error_reduce{postfix}`, `mAP_truncate{postfix}` (with its recalls and precisions), `reduce_gain{postfix}` = mAP_reduce -
mAP_truncate (a list where mAP is a list) and `reduce_bits`, `reduce_blocks`, `reduce_method` are added to the results and to
`history.json` beside the call's own keys.  Single process only (NotImplementedError for RowShards or more than one rank, as the
other re-scored rankings).  It extends the ITQ evaluator, and through it every other one, so their keys keep working beside it;
`itq_eval` in the same run is refused (its rotated call would be reduced once more).
"""
from __future__ import annotations

import torch

import utils.hashing
from concepthash_amd import retrieval as rt
from experiments.itq_eval import ItqEvaluation
from experiments.rank_rescoring import main_under_rank

KEYS = ("mAP_reduce", "recalls_reduce", "precisions_reduce")
TRUNCATE_KEYS = ("mAP_truncate", "recalls_truncate", "precisions_truncate")


def check_reduce_settings(bits, method, blocks, iters, ncontext: int):
    """(`reduce_bits`, `reduce_method`, `reduce_blocks`, `reduce_iters`) of a `reduce_eval` run (ValueError otherwise)"""
    if bits is None:
        raise ValueError("reduce_eval: reduce_bits=<m>, the code length to reduce to, is required (no default)")
    if isinstance(bits, bool) or not isinstance(bits, int) or bits < 1:
        raise ValueError(f"reduce_eval: reduce_bits must be an int >= 1, got {bits!r}")
    method = "pca-itq" if method is None else str(method)
    if method not in rt.REDUCE_METHODS:
        raise ValueError(f"reduce_eval: reduce_method must be one of {rt.REDUCE_METHODS}, got {method!r}")
    blocks = int(ncontext) if blocks is None else blocks
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 1:
        raise ValueError(f"reduce_eval: reduce_blocks must be an int >= 1, got {blocks!r}")
    iters = 50 if iters is None else iters
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"reduce_eval: reduce_iters must be an int >= 1, got {iters!r}")
    return bits, method, blocks, iters


def truncated_columns(width: int, bits: int, blocks: int) -> torch.Tensor:
    """the first bits / blocks columns of every block of `width` columns in `blocks` blocks"""
    s, t = width // blocks, bits // blocks
    return (torch.arange(blocks)[:, None] * s + torch.arange(t)[None, :]).reshape(-1)


def reduced_pair(db_codes, test_codes, bits: int, blocks: int, iters: int, method: str):
    """Fit on the database codes, reduce both sets through the one chain -> (db, test, the fit).  Settings that do not suit the
    evaluated width: ValueError."""
    width = int(db_codes.shape[1])
    try:
        rt.check_reduction(width, bits, blocks, method)
    except ValueError as e:
        raise ValueError(f"reduce_eval: {e} (the evaluated code width is {width})") from None
    dev = utils.hashing._device()
    db = torch.as_tensor(db_codes).to(dev, torch.float32).contiguous()
    test = torch.as_tensor(test_codes).to(dev, torch.float32).contiguous()
    fit = rt.fit_reduction(db, bits, blocks, iters, method)
    return rt.project_codes(db, fit["mean"], fit["A"], blocks), rt.project_codes(test, fit["mean"], fit["A"], blocks), fit


class ReduceEvaluation(ItqEvaluation):
    def main(self):
        cfg = self.config
        if not (cfg.get("reduce_eval") and cfg.get("compute_mAP") and cfg.exp != "extract"):
            return super().main()
        if cfg.get("itq_eval"):
            raise ValueError("reduce_eval together with itq_eval is not built: reduce_method=pca-itq holds its own rotation")
        bits, method, blocks, iters = check_reduce_settings(cfg.get("reduce_bits"), cfg.get("reduce_method"), cfg.get("reduce_blocks"),
                                                            cfg.get("reduce_iters"), int(cfg.model.ncontext))
        fits = []                           # the fit of every repeated call, in the order of the calls

        def recode(db_codes, db_labels, test_codes, test_labels):
            utils.hashing._single_process("hamming after reduce_eval", db_codes, db_labels, test_codes, test_labels)
            db, test, fit = reduced_pair(db_codes, test_codes, bits, blocks, iters, method)
            fits.append(fit)
            return db, test

        def truncate(db_codes, db_labels, test_codes, test_labels):
            cols = truncated_columns(int(db_codes.shape[1]), bits, blocks)
            db, test = torch.as_tensor(db_codes), torch.as_tensor(test_codes)
            return db[:, cols.to(db.device)].contiguous(), test[:, cols.to(test.device)].contiguous()

        def finish(res, calls):
            for (mAP, postfix, red), fit in zip(calls, fits):
                res["reduce_iters_run" + postfix] = fit["iters_run"]
                res["reduce_explained" + postfix] = fit["explained_share"]
                res["quantisation_error_reduce" + postfix] = fit["qerr_after"]
                cut = res["mAP_truncate" + postfix]
                res["reduce_gain" + postfix] = [r - c for r, c in zip(red[0], cut)] if isinstance(cut, list) else red[0] - cut
            res["reduce_bits"], res["reduce_blocks"], res["reduce_method"] = bits, blocks, method

        return main_under_rank(self, super().main, "reduce_eval", {}, ("tie_bracket", "tie_expected", "radii", "rank", "weight_bits", "margin", "shortlist"),
                               f"Hamming, {bits} bits after {method} in {blocks} blocks", "reduce", KEYS, finish=finish, recode=recode,
                               also=[(TRUNCATE_KEYS, truncate, f"Hamming, the first {bits // blocks} bits of {blocks} blocks")])
