"""`exp=search`: image or text queries -> ranked database hits of a finished run, optionally by chosen concepts.

    python main_v2.py --config-name search.yaml logdir=<run> dataset=<name> [query=test] [k=10] [radius=2] [concepts=[0,2]]
        [query_margin=0.0] [rank=hamming|asymmetric|ternary|cosine|euclidean|dot] [shortlist=1000] [weight_bits=8] [index=<file>] [rebuild_index=false] [save_attention=false]
        [query_text="painted bunting" | query_text=[...] | query_text_file=<file> | query=classes] [prompt_prefix=...] [text_model=<dir>]
        [only_classes=[3,"Painted Bunting"]] [exclude_classes=[...]] [exclude_self=true] [same_class=only|exclude]
        [rotate=itq] [rotate_blocks=<int>] [rotate_iters=50]
        [reduce=pca-itq|pca reduce_bits=<m>] [reduce_blocks=<int>] [reduce_iters=50]

Reduction ("reduction"): `reduce=pca-itq reduce_bits=<m>` fits a block-wise PCA of the database's real-valued codes
to `m` dimensions, and behind it a rotation (`reduce=pca`: none), once (`GalleryIndex.fit_reduction`; `reduce_blocks` blocks, the run's
ncontext by default), keeps it in the index -- then an ordinary index of `m` bits -- and reduces every query; an index built under another
`reduce` setting is stale, and `reduce` together with `rotate` is a ValueError.  `results.json` records it under "reduction".

Learned rotation ("learned rotation"): `rotate=itq` fits a block-diagonal rotation to the database's real-valued
codes once (`GalleryIndex.fit_rotation`; `rotate_blocks` blocks, the run's ncontext by default, at most `rotate_iters` updates), keeps it in
the index and rotates every query; an index built under another `rotate` setting is stale.  `results.json` records it under "rotation".

Filtered search ("filtered search"; rank hamming, asymmetric or ternary, k <= 128): `only_classes` / `exclude_classes`
admit only database rows of (not of) these classes -- ids, or names of the dataset's class_names.txt; `exclude_self=true` keeps an image
query that IS a database image (query=db, or a path the index holds) from returning its own row; `same_class=only|exclude` keeps every
labelled query to hits of its own class (of every other class).  `results.json` records the filter under "filter".

Text queries ("text query") become codes through the CLIP text tower and the run's own `text_projection`
(`concepthash_amd.text.TextQueryEncoder`) and go through the same `GalleryIndex.search` call as image codes, never shifted by an index's mean.

The run's config and checkpoint are loaded exactly as `exp=validation` loads them.  The database split is encoded once
(`trainer.inference_one_epoch("db", True)`) into a `concepthash_amd.search.GalleryIndex` file -- `<logdir>/index_<best|last>.pth` unless
`index=` names another -- and later invocations load that file instead of reading the database images, as long as its checkpoint
fingerprint and code length still match.  `query` is a split of the dataset (`test`, `db`), a directory of image files (sorted by name,
not recursive, no labels), a list file in the dataset's own format, or one image file; queries go through the evaluation transform
chain of the dataset config and the evaluation loader.  Output: `<search_logdir>/results.json` (schema: INTEGRATION.md, "Search
results") and, with `save_attention=true`, `concept_attention.npy` [Nq, Q, gh, gw] fp32 -- the head mean of the last layer's
concept-token attention over the patch grid.
"""
from __future__ import annotations

import copy
import json
import math
import os
import time

import numpy as np
import torch
import yaml

import engine
from concepthash_amd import retrieval as rt
from concepthash_amd.config import DictConfig, instantiate, to_container
from concepthash_amd.search import GalleryIndex, StaleIndexError, checkpoint_fingerprint

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".webp", ".ppm", ".tif", ".tiff", ".gif")
SPLITS = ("test", "db")
PRINT_QUERIES = 3


def _label_ids(labels: torch.Tensor):
    """[N, C] indicator rows -> [N] int64 class ids when every row names exactly one class, else uint8 indicator rows; 1-D ids pass"""
    if labels.dim() == 1:
        return labels.to(torch.int64)
    hot = labels != 0
    if bool((hot.sum(1) == 1).all()):
        return hot.int().argmax(1).to(torch.int64)
    return hot.to(torch.uint8)


def class_name_file(config) -> str:
    """`class_names.txt` of the dataset folder this invocation names"""
    return os.path.join(str(config.data_dir), str(config.dataset.data_folder), "class_names.txt")


def text_request(config):
    """The text queries of an invocation, from its config alone (no model, no GPU): None when it asks for image queries, else a dict
    with `prompts` (the strings the tokeniser gets, prefix included), `labels` (class ids for `query=classes`, else None), `prefix`, `run_prefix`
    (the run's own, for the tower check) and `text_model`.  `query_text` (one string or a list) / `query_text_file` (one prompt per line) are appended to the prefix;
    `query=classes` is `trainers.orthohash.class_prompts` of the dataset's class_names.txt under that prefix."""
    from concepthash_amd.text import text_query_settings
    from trainers.orthohash import class_prompts
    query = str(config.get("query", "test") or "test")
    given = [k for k in ("query_text", "query_text_file") if config.get(k) is not None]
    if not given and query != "classes":
        return None
    if len(given) > 1 or (given and query != "test"):
        raise ValueError(f"text queries come from ONE of query_text, query_text_file and query=classes; got {given} with query='{query}'")
    if config.get("save_attention"):
        raise ValueError("save_attention=true needs image queries: a text query has no image whose patches the concept tokens attend to")
    source, prefix = text_query_settings(config, config.get("text_model"), config.get("prompt_prefix"))
    labels = None
    if query == "classes":
        path = class_name_file(config)
        if not os.path.isfile(path):
            raise ValueError(f"query=classes reads one class name per line from {path}, which does not exist")
        prompts = class_prompts(path, prefix)
        labels = list(range(len(prompts)))
    elif given[0] == "query_text":
        qt = config.query_text
        prompts = [prefix + str(p) for p in ([qt] if isinstance(qt, str) else list(qt))]
    else:
        path = str(config.query_text_file)
        if not os.path.isfile(path):
            raise ValueError(f"query_text_file={path} does not exist")
        with open(path, encoding="utf-8") as f:
            prompts = [prefix + line.strip() for line in f if line.strip()]
    if not prompts:
        raise ValueError(f"{'query=classes' if query == 'classes' else given[0]} gives no prompt")
    # the tower check (center_agreement) rebuilds the run's centres: under the run's own prefix, whatever the queries use
    run_prefix = text_query_settings(config, config.get("text_model"))[1]
    return {"prompts": prompts, "labels": labels, "prefix": prefix, "run_prefix": run_prefix, "text_model": source}


def filter_request(config):
    """The filter of an invocation, from its config alone (no model, no GPU): None without one of the four keys, else a dict with
    `only_classes` / `exclude_classes` (class ids or None; names are looked up in the dataset's class_names.txt), `exclude_self` (bool)
    and `same_class` (None, "only" or "exclude").  An error names the key."""
    only, out = config.get("only_classes"), config.get("exclude_classes")
    self_, same = bool(config.get("exclude_self")), config.get("same_class")
    if only is None and out is None and not self_ and same is None:
        return None
    if same is not None and str(same) not in ("only", "exclude"):
        raise ValueError(f"same_class must be only or exclude, got {same!r}")
    if same is not None and self_:
        raise ValueError("same_class with exclude_self=true is not built: a query has ONE group per search (its class, or its own row)")
    names = None

    def ids(key, values):
        nonlocal names
        got = []
        for v in ([values] if isinstance(values, (str, int)) else list(values)):
            if isinstance(v, int) or str(v).lstrip("-").isdigit():
                got.append(int(v))
                continue
            if names is None:
                path = class_name_file(config)
                if not os.path.isfile(path):
                    raise ValueError(f"{key}: the class name {v!r} is looked up in {path}, which does not exist")
                with open(path, encoding="utf-8") as f:
                    names = [line.strip() for line in f]
            if str(v) not in names:
                raise ValueError(f"{key}: unknown class name {v!r} (not a line of {class_name_file(config)})")
            got.append(names.index(str(v)))
        if any(c < 0 for c in got):
            raise ValueError(f"{key}: class ids must be >= 0, got {got}")
        return got

    return {"only_classes": ids("only_classes", only) if only is not None else None,
            "exclude_classes": ids("exclude_classes", out) if out is not None else None,
            "exclude_self": self_, "same_class": str(same) if same is not None else None}


def rotation_request(config):
    """The learned rotation of an invocation, from its config alone (no model, no GPU): None without `rotate`, else a dict with `method`
    ("itq"), `blocks` (rotate_blocks, or the run's ncontext) and `iters`.  An error names the key."""
    method, blocks, iters = config.get("rotate"), config.get("rotate_blocks"), config.get("rotate_iters")
    if method is None or str(method) in ("", "none", "None"):
        if blocks is not None:
            raise ValueError(f"rotate_blocks={blocks!r} without rotate=itq")
        return None
    if str(method) != "itq":
        raise ValueError(f"rotate must be itq (or left out), got {method!r}")
    nbit, ncontext = int(config.model.nbit), int(config.model.ncontext)
    if blocks is None:
        blocks = ncontext
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 1 or nbit % blocks:
        raise ValueError(f"rotate_blocks must be an int >= 1 that divides nbit = {nbit}, got {blocks!r}")
    iters = 50 if iters is None else iters
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"rotate_iters must be an int >= 1, got {iters!r}")
    return {"method": "itq", "blocks": blocks, "iters": iters}


def reduction_request(config):
    """The reduction of an invocation, from its config alone (no model, no GPU): None without `reduce`, else a dict with `method`
    ("pca-itq" | "pca"), `bits` (reduce_bits: required), `blocks` (reduce_blocks, or the run's ncontext) and `iters`.  An error names
    the key; `reduce` beside `rotate` is refused."""
    method, bits = config.get("reduce"), config.get("reduce_bits")
    blocks, iters = config.get("reduce_blocks"), config.get("reduce_iters")
    if method is None or str(method) in ("", "none", "None"):
        if bits is not None or blocks is not None:
            raise ValueError(f"reduce_bits={bits!r} / reduce_blocks={blocks!r} without reduce=pca-itq|pca")
        return None
    if str(method) not in rt.REDUCE_METHODS:
        raise ValueError(f"reduce must be one of {rt.REDUCE_METHODS} (or left out), got {method!r}")
    rotate = config.get("rotate")
    if rotate is not None and str(rotate) not in ("", "none", "None"):
        raise ValueError(f"reduce={method} together with rotate={rotate} is not built: reduce=pca-itq holds its own rotation")
    if bits is None:
        raise ValueError(f"reduce={method} needs reduce_bits=<m>, the code length to reduce to (no default)")
    nbit, ncontext = int(config.model.nbit), int(config.model.ncontext)
    if blocks is None:
        blocks = ncontext
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 1 or nbit % blocks:
        raise ValueError(f"reduce_blocks must be an int >= 1 that divides nbit = {nbit}, got {blocks!r}")
    if isinstance(bits, bool) or not isinstance(bits, int) or not blocks <= bits <= nbit or bits % blocks or bits % ncontext:
        raise ValueError(f"reduce_bits must be an int in [reduce_blocks, nbit] = [{blocks}, {nbit}], a multiple of reduce_blocks = {blocks} "
                         f"and of ncontext = {ncontext}, got {bits!r}")
    iters = 50 if iters is None else iters
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"reduce_iters must be an int >= 1, got {iters!r}")
    return {"method": str(method), "bits": bits, "blocks": blocks, "iters": iters}


class SearchExperiment:
    def __init__(self, config: DictConfig):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("exp=search under a multi-rank process group is not built: a query tool gains nothing from sharding; "
                                      "run it as a single process")
        self.start_time = time.time()
        self.config = config
        self.query = str(config.get("query", "test") or "test")
        self.text = text_request(config)              # None: image queries.  Argument errors surface here, before anything is loaded
        self.filter = filter_request(config)          # None: every row may be a hit
        self.rotation = rotation_request(config)      # None: the codes are searched as the model gives them
        self.reduction = reduction_request(config)    # None: at the length the model gives them
        if self.filter is not None and self.filter["exclude_self"] and self.text is not None:
            raise ValueError("exclude_self=true needs image queries: a text query is no database row")
        engine.seeding(config["seed"])
        self.timing = {}
        logdir = config.logdir
        modelfn = "last" if config.get("use_last") else "best"
        self.checkpoint = f"{logdir}/models/{modelfn}.pth"
        self.index_path = str(config.get("index") or os.path.join(logdir, f"index_{modelfn}.pth"))
        self.search_logdir = str(config.search_logdir)
        os.makedirs(self.search_logdir, exist_ok=True)
        with open(os.path.join(self.search_logdir, "search_config.yaml"), "w") as f:
            yaml.safe_dump(to_container(config), f)
        self.nbit, self.ncontext = int(config.model.nbit), int(config.model.ncontext)
        # rank=ternary ranks against the database's own ternary codes: the index then carries the mask plane of index_margin
        self.ternary = str(config.get("rank", "hamming") or "hamming") == "ternary"
        self.index_margin = rt.check_margin(config.get("index_margin", 0.0) or 0.0, "index_margin") if self.ternary else None
        # rank=cosine | euclidean | dot rank the real-valued codes themselves: the index then carries them as its real plane
        # (so do rotate=itq and reduce=...: they are fitted to them)
        self.dense = str(config.get("rank", "hamming") or "hamming") in rt.DENSE_METRICS

        # the index first: whether the database split has to be encoded decides what is loaded
        self.fingerprint = self._phase("fingerprint", checkpoint_fingerprint, self.checkpoint)
        self.index, self.index_note = None, "built: no index file"
        if config.get("rebuild_index"):
            self.index_note = "built: rebuild_index"
        elif os.path.exists(self.index_path):
            try:
                self.index = self._phase("index_load", GalleryIndex.load, self.index_path, self.fingerprint, self.nbit)
                self._check_index_settings(self.index)
                self.index_note = "loaded"
            except StaleIndexError as e:
                print(f"Stale index: {e}")
                self.index, self.index_note = None, f"built: stale index ({e})"

        trainer = instantiate(config.trainer, config)
        if self.text is None or self.index is None:   # text queries over a valid index read no image: no dataset is loaded at all
            self._phase("datasets", trainer.load_dataset, load_db=self.index is None or self.query == "db")
            self._phase("loaders", trainer.load_dataloader)
        trainer.load_for_inference(logdir)
        self._phase("model_build", trainer.load_model)
        trainer.load_criterion()
        self._phase("checkpoint", trainer.load_model_state, self.checkpoint)
        self._phase("to_device", trainer.to_device)
        self.trainer = trainer

    def _phase(self, name, fn, *a, **k):
        t0 = time.perf_counter()
        out = fn(*a, **k)
        self.timing[name] = round(self.timing.get(name, 0.0) + time.perf_counter() - t0, 3)
        return out

    # ---- index -------------------------------------------------------------------------------------------------------------------
    def _transform_settings(self):
        ds = self.config.dataset
        return {"resize": int(ds.get("resize", 256)), "crop": int(ds.get("crop", 224)), "norm": int(ds.get("norm", 3))}

    def _check_index_settings(self, index: GalleryIndex):
        """what the fingerprint does not cover: the code layout, the evaluation transform and the zero-mean switch of THIS invocation"""
        want_mean = bool(self.config.get("zero_mean_eval"))
        if index.ncontext != self.ncontext or index.transform != self._transform_settings() or (index.mean is not None) != want_mean:
            raise StaleIndexError(f"{self.index_path} was built with ncontext = {index.ncontext}, transform {index.transform}, "
                                  f"zero_mean_eval = {index.mean is not None}; this run asks for ncontext = {self.ncontext}, "
                                  f"{self._transform_settings()}, zero_mean_eval = {want_mean}: rebuild the index (rebuild_index=true)")
        if self.ternary and (index.mask is None or index.margin != self.index_margin):
            have = "no mask plane" if index.mask is None else f"the mask plane of index_margin = {index.margin}"
            raise StaleIndexError(f"{self.index_path} holds {have}; rank=ternary index_margin={self.index_margin} needs its own: rebuild the "
                                  f"index (rebuild_index=true)")
        if self.dense and index.real is None:
            raise StaleIndexError(f"{self.index_path} holds no real plane; rank={self.config.get('rank')} ranks the real-valued codes and "
                                  f"needs it: rebuild the index (rebuild_index=true)")
        have = None if index.rotation is None else (index.rotation_info.get("method"), index.rotation_blocks)
        want = None if self.rotation is None else (self.rotation["method"], self.rotation["blocks"])
        if have != want:
            raise StaleIndexError(f"{self.index_path} was built under rotate = {have}; this run asks for {want} ((method, blocks); None: no "
                                  f"rotation): rebuild the index (rebuild_index=true)")
        have = None if index.reduce_A is None else (index.reduce_info.get("method"), index.nbit, index.reduce_blocks)
        want = None if self.reduction is None else (self.reduction["method"], self.reduction["bits"], self.reduction["blocks"])
        if have != want:
            raise StaleIndexError(f"{self.index_path} was built under reduce = {have}; this run asks for {want} ((method, bits, blocks); "
                                  f"None: no reduction): rebuild the index (rebuild_index=true)")

    def _build_index(self) -> GalleryIndex:
        _, out = self._phase("encode_db", self.trainer.inference_one_epoch, "db", True)
        codes = out["codes"].to(torch.float32)
        mean = None
        if self.config.get("zero_mean_eval"):         # the database mean, applied to both sets (experiments/test_hashing.py)
            mean = codes.mean(dim=0, keepdim=True)
            codes = codes - mean
            mean = mean[0]
        ds = self.trainer.dataset["db"]
        items = getattr(ds, "items", None)             # list-file datasets name their files; the synthetic ones have none
        codes = codes.to(self.trainer.device)
        mask = rt.confidence_mask(codes, self.index_margin) if self.ternary else None
        index = GalleryIndex(rt.pack_sign(codes), self.nbit, self.ncontext, labels=_label_ids(out["labels"]),
                             paths=[p for p, _ in items] if items is not None else None,
                             data_root=getattr(ds, "root", None) if items is not None else None, mean=mean,
                             transform=self._transform_settings(), fingerprint=self.fingerprint, mask=mask, margin=self.index_margin,
                             real=codes if self.dense or self.rotation is not None or self.reduction is not None else None)
        if self.reduction is not None:
            red = self.reduction
            index = self._phase("fit_reduction", index.fit_reduction, red["bits"], red["blocks"], red["iters"], red["method"])
        if self.rotation is not None:
            index = self._phase("fit_rotation", index.fit_rotation, self.rotation["blocks"], self.rotation["iters"])
        self._phase("index_save", index.save, self.index_path)
        return index

    # ---- queries -----------------------------------------------------------------------------------------------------------------
    def _path_dataset(self, items, labelled, root=None):
        """The test split's dataset node -- its evaluation transform list and GPU data path -- over other files"""
        node = copy.deepcopy(self.config.dataset.test_dataset)
        if str(node.get("_target_", "")) != "utils.datasets.HashingDataset":
            raise ValueError(f"query='{self.query}' names image files, but dataset '{self.config.get('dataset_name', '')}' is not a list-file "
                             f"image dataset ({node.get('_target_')}); its queries are the splits {SPLITS}")
        if root is not None:
            node["root"] = root
        if not labelled:
            node["target_transform"] = None
        return instantiate(node, items=items)

    def _query_loader(self):
        """-> (loader, names of the queries or None, whether they carry labels)"""
        q = self.query
        if q in SPLITS:
            ds = self.trainer.dataset[q]
            items = getattr(ds, "items", None)
            return self.trainer.dataloader[q], ([p for p, _ in items] if items is not None else None), True
        if os.path.isdir(q):
            files = sorted(f for f in os.listdir(q) if f.lower().endswith(IMAGE_EXTENSIONS) and os.path.isfile(os.path.join(q, f)))
            if not files:
                raise ValueError(f"query directory {q} holds no image file ({', '.join(IMAGE_EXTENSIONS)})")
            names = [os.path.join(os.path.abspath(q), f) for f in files]
            ds = self._path_dataset([(p, -1) for p in names], labelled=False)
            labelled = False
        elif os.path.isfile(q) and q.lower().endswith(IMAGE_EXTENSIONS):
            names = [os.path.abspath(q)]
            ds = self._path_dataset([(names[0], -1)], labelled=False)
            labelled = False
        elif os.path.isfile(q):
            from utils.datasets import read_list
            items = read_list(q)
            if not items:
                raise ValueError(f"query list file {q} is empty")
            names = [p for p, _ in items]
            ds = self._path_dataset(items, labelled=True)
            labelled = True
        else:
            raise ValueError(f"query='{q}' is neither a split ({', '.join(SPLITS)}) nor an existing directory, list file or image file")
        bs = self.config.batch_size
        if getattr(ds, "gpu_decode", False) and not getattr(ds, "file_workers", 0):
            bs = max(bs, int(self.config.get("eval_batch_min", 256) or 0))
        return engine.dataloader(ds, bs, shuffle=False, drop_last=False), names, labelled

    def _encode_queries(self, loader, want_attention):
        tr = self.trainer
        tr.model.eval()
        tr.criterion.eval()
        before = getattr(tr.model, "return_concept_attention", False)
        if want_attention:
            tr.model.return_concept_attention = True
        codes, labels, attn = [], [], []
        try:
            for data in tr.iterate_loader(loader):
                with torch.no_grad():
                    (_, lab, _), out = tr.compute_features_one_batch(data)
                codes.append(out["codes"])
                labels.append(lab)
                if want_attention:
                    a = out["concept_attention"].to(torch.float32).mean(1)          # [B, heads, Q, Np] -> head mean
                    side = math.isqrt(a.shape[-1])
                    if side * side != a.shape[-1]:
                        raise RuntimeError(f"concept attention over {a.shape[-1]} patches is not a square grid")
                    attn.append(a.reshape(a.shape[0], a.shape[1], side, side))
        finally:
            tr.model.return_concept_attention = before
        return torch.cat(codes), torch.cat(labels), (torch.cat(attn) if attn else None)

    def _encode_text(self):
        """-> (query codes [N, nbit] of the prompts, share of the run's centre entries the same tower rebuilds from class_names.txt or
        None without that file)"""
        from concepthash_amd.text import TextQueryEncoder
        model = self.trainer.model
        model.eval()
        names = class_name_file(self.config)
        with TextQueryEncoder(model, self.text["text_model"], prefix="") as enc, torch.no_grad():   # the prompts carry their prefix
            codes = enc.text_codes(self.text["prompts"])
            agreement = enc.center_agreement(names, self.text["run_prefix"]) if os.path.isfile(names) else None
        return codes, agreement

    def _filter_arguments(self, index: GalleryIndex, names, labelled: bool, q_labels: torch.Tensor) -> dict:
        """what `GalleryIndex.search` takes for this invocation's filter (`filter_request`)"""
        f = self.filter
        args = {}
        if f["only_classes"] is not None:
            args["labels_in"] = f["only_classes"]
        if f["exclude_classes"] is not None:
            args["labels_out"] = f["exclude_classes"]
        if f["exclude_self"]:
            n = q_labels.shape[0] if names is None else len(names)
            if self.query == "db":                       # query i is database row i
                rows = list(range(n))
            elif names is None or index.paths is None:
                rows = [-1] * n                          # nothing to compare: no query is a known database row
            else:
                at = {}
                for r, p in enumerate(index.paths):
                    at.setdefault(p, r)
                    at.setdefault(os.path.abspath(index.resolve(p)), r)
                rows = [at.get(p, at.get(os.path.abspath(index.resolve(p)), -1)) for p in names]
            args.update(query_group=torch.tensor(rows, dtype=torch.int64), group_mode="exclude", group_by="row")
        if f["same_class"] is not None:
            ids = _label_ids(q_labels.cpu()) if labelled else None
            if ids is None or ids.dim() != 1 or ids.shape[0] == 0:
                raise ValueError(f"same_class={f['same_class']} needs labelled queries with one class each; these queries carry " +
                                 ("no labels" if ids is None or ids.shape[0] == 0 else "indicator rows"))
            args.update(query_group=ids.to(torch.int64), group_mode=f["same_class"], group_by="labels")
        return args

    # ---- main --------------------------------------------------------------------------------------------------------------------
    def main(self):
        cfg = self.config
        k = int(cfg.get("k", 10))
        concepts = cfg.get("concepts")
        concepts = [int(c) for c in concepts] if concepts is not None else None
        margin = float(cfg.get("query_margin", 0.0) or 0.0)
        rank = str(cfg.get("rank", "hamming") or "hamming")
        weight_bits = int(cfg.get("weight_bits", 8) or 8)
        radius = cfg.get("radius")
        radius = int(radius) if radius is not None else None
        shortlist = cfg.get("shortlist")
        shortlist = int(shortlist) if shortlist is not None else None
        print("Search Start")
        index = self.index if self.index is not None else self._build_index()
        index = index.to(self.trainer.device)
        agreement = None
        if self.text is not None:
            names, labelled, attn = self.text["prompts"], self.text["labels"] is not None, None
            q_codes, agreement = self._phase("encode_query", self._encode_text)
            q_labels = torch.tensor(self.text["labels"] if labelled else [], dtype=torch.int64)
        else:
            loader, names, labelled = self._query_loader()
            q_codes, q_labels, attn = self._phase("encode_query", self._encode_queries, loader, bool(cfg.get("save_attention")))
        res = self._phase("search", index.search, q_codes, k, concepts, margin, rank, weight_bits, radius, mean_shift=self.text is None,
                          shortlist=shortlist, **(self._filter_arguments(index, names, labelled, q_labels) if self.filter is not None else {}))
        t0 = time.perf_counter()
        q_ids = _label_ids(q_labels.cpu()) if labelled else None
        idx, dist, cdist = res["idx"].tolist(), res["dist"].tolist(), res["concept_dist"].tolist()
        bits = res["bits"].tolist()
        dist_max = res["dist_max"].tolist() if "dist_max" in res else bits      # the distance of a row that disagrees on every unmasked bit
        dense = rank in rt.DENSE_METRICS
        if dense:
            dist_max = [None] * len(idx)                                        # a real-valued distance has no such row
        dist_bits = res["dist_bits"].tolist() if "dist_bits" in res else None   # rank=ternary: the distance is in half bits
        hit_labels = res["labels"].cpu() if res["labels"] is not None else None
        queries = []
        for i in range(len(idx)):
            ql = q_ids[i] if q_ids is not None else None
            hits = []
            for r in range(k):
                if idx[i][r] < 0:
                    break
                hl = hit_labels[i, r] if hit_labels is not None else None
                relevant = None
                if ql is not None and hl is not None and ql.dim() == hl.dim():
                    relevant = bool(ql == hl) if hl.dim() == 0 else bool((ql & hl).any())
                rel_path = res["paths"][i][r] if res["paths"] is not None else None
                hits.append({"rank": r + 1, "index": idx[i][r], "path": index.resolve(rel_path), "distance": dist[i][r],
                             "label": hl.tolist() if hl is not None else None, "relevant": relevant, "concept_distances": cdist[i][r]})
                if dist_bits is not None:
                    hits[-1]["distance_bits"] = dist_bits[i][r]
            queries.append({"query": names[i] if names is not None else i, "label": ql.tolist() if ql is not None else None,
                            "unmasked_bits": bits[i], "distance_max": dist_max[i], "hits": hits})
        self.timing["results"] = round(time.perf_counter() - t0, 3)
        out = {"k": k, "radius": radius, "shortlist": shortlist, "concepts": concepts, "query_margin": margin, "rank": rank, "weight_bits": weight_bits, "index_margin": index.margin, "nbit": index.nbit, "ncontext": index.ncontext,
               "index": os.path.abspath(self.index_path), "index_status": self.index_note, "index_rows": len(index),
               "checkpoint": self.fingerprint, "query_kind": "image" if self.text is None else "text",
               "query": self.query if self.text is None else list(self.text["prompts"]),
               "prefix": None if self.text is None else self.text["prefix"], "text_model": None if self.text is None else self.text["text_model"],
               "filter": None if self.filter is None else dict(self.filter, rows_admitted=int(res["rows_admitted"])),
               "rotation": None if index.rotation is None else dict(index.rotation_info, keeps_concepts=index.keeps_concepts),
               "reduction": None if index.reduce_A is None else dict(index.reduce_info, keeps_concepts=index.keeps_concepts),
               "center_agreement": agreement, "mean_shift": self.text is None and index.mean is not None, "queries": queries,
               "timing_s": dict(self.timing, since_start=round(time.time() - self.start_time, 3))}
        with open(os.path.join(self.search_logdir, "results.json"), "w") as f:
            json.dump(out, f)
        if attn is not None:
            np.save(os.path.join(self.search_logdir, "concept_attention.npy"), attn.cpu().numpy().astype(np.float32))
        what = "the whole code" if concepts is None else f"concepts {concepts}"
        print(f"{len(queries)} queries x top {k} of {len(index)} database rows, ranked by {what}, " +
              (f"{rank} distance of the real-valued codes" + (f" over a Hamming shortlist of {shortlist}" if shortlist is not None else "") if dense else "Hamming distance" if rank == "hamming" else f"ternary distance in half bits (database margin {index.margin})" if rank == "ternary"
               else f"asymmetric distance ({weight_bits}-bit |code| weights)") +
              (f", ignoring bits with |code| <= {margin}" if margin > 0 else "") + (f", within {radius} bits" if radius is not None else "") + f"; index {self.index_note}")
        for e in queries[:PRINT_QUERIES]:
            print(f"query {e['query']}" + (f" (label {e['label']})" if e["label"] is not None and not isinstance(e["label"], list) else "") +
                  f": {e['unmasked_bits']} bits" + ("" if dense else f", distance <= {e['distance_max']}"))
            for h in e["hits"]:
                mark = "" if h["relevant"] is None else (" +" if h["relevant"] else " -")
                print(f"  {h['rank']:3d}. d=" + (f"{h['distance']:.6g}" if dense else f"{h['distance']:3d}") + f" per concept {h['concept_distances']}  #{h['index']}" +
                      (f" {h['path']}" if h["path"] else "") + mark)
        print("Phases (s): " + ", ".join(f"{n} {v:.2f}" for n, v in self.timing.items()))
        print(f"Done: {self.search_logdir}")
        self.results = out
        return out
