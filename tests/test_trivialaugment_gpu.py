"""TrivialAugmentWide training chain on the GPU (csrc/augment.hip through GpuPreprocess): Resize(256, bilinear) -> RandomHorizontalFlip
-> TrivialAugmentWide(bicubic) -> CenterCrop(224) -> ToTensor -> normalize equals the PIL chain of utils.transforms with the same draws,
BIT FOR BIT in fp32 (bf16: its RNE rounding), for every op at bins {0, 1, 15, 20, 30} and both signs, on landscape, portrait, square
(rotate's +-90 transpose path) and tiny up-scaled images and on the host route; through both GPU data paths and the trainer's loader."""
import numpy as np
import pytest
import torch
from PIL import Image

from test_preprocess import _image, _write_dataset
from test_trivialaugment_cpu import _ta_chain

pytestmark = pytest.mark.gpu

SIZES = [(300, 400), (400, 300), (300, 300), (30, 40)]


def _combos():
    from utils.transforms import TA_OPS, ta_augmentation_space
    space = ta_augmentation_space(31)
    out = []
    for op, name in enumerate(TA_OPS):
        mags, signed = space[name]
        if mags.ndim == 0:
            out.append((op, 0.0))
            continue
        for b in (0, 1, 15, 20, 30):
            m = float(mags[b].item())
            out += [(op, m), (op, -m)] if signed else [(op, m)]
    return out


def _pil(img, flip, op, m, norm=3):
    from utils import transforms as T
    img = T.Resize(256)(Image.fromarray(img))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = T.TrivialAugmentWide(interpolation=Image.BICUBIC).apply(img, op, m)
    return T.normalize_transform(norm)(T.ToTensor()(T.CenterCrop(224)(img)))


def test_every_op_bin_and_sign_equals_the_pil_chain():
    from concepthash_amd.preprocess import GpuPreprocess
    from utils.transforms import _NORMS
    dev = torch.device("cuda:0")
    pre32 = GpuPreprocess(256, 224, *_NORMS[3], out_dtype=torch.float32, device=dev)
    pre16 = GpuPreprocess(256, 224, *_NORMS[3], out_dtype=torch.bfloat16, device=dev)
    combos = _combos()
    assert len(combos) == 103
    for k, (h, w) in enumerate(SIZES):
        img = _image(h, w, k)
        flips = [(i + k) % 2 == 1 for i in range(len(combos))]
        want = torch.stack([_pil(img, f, op, m) for f, (op, m) in zip(flips, combos)])
        pixels = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (len(combos),) + img.shape))).reshape(-1).to(dev)
        sizes = [(h, w)] * len(combos)
        ta = torch.tensor(combos, dtype=torch.float64)
        got = pre32(pixels, sizes, flips=flips, ta=ta).cpu()
        bad = [(combos[i], flips[i]) for i in range(len(combos)) if not torch.equal(got[i], want[i])]
        assert not bad, ((h, w), bad[:8])
        assert torch.equal(pre16(pixels, sizes, flips=flips, ta=ta).cpu(), want.to(torch.bfloat16)), (h, w)
    assert pre32.host_routed == 0
    # the host route (more filter taps than the kernels hold: lowered here so that a small image takes it) is the PIL chain itself
    pre32.max_taps = 3
    img = _image(400, 300, 9)
    sub = [(1, 0.33), (5, 90.0), (12, 0.0), (0, 0.0)]
    pixels = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (len(sub),) + img.shape))).reshape(-1).to(dev)
    got = pre32(pixels, [(400, 300)] * len(sub), flips=[True, False, True, False], ta=torch.tensor(sub, dtype=torch.float64)).cpu()
    assert pre32.host_routed == len(sub)
    for i, (op, m) in enumerate(sub):
        assert torch.equal(got[i], _pil(img, i % 2 == 0, op, m))


def test_both_gpu_data_paths_equal_the_cpu_loader(tmp_path):
    """gpu_preprocess (decoded images) and gpu_decode (undecoded files): the loader's draws with the CPU chain's seed give the CPU
    dataset's tensors, fp32 equal and bf16 the RNE rounding."""
    from concepthash_amd.jpeg import GpuJpegDecoder
    from concepthash_amd.preprocess import GpuPreprocess
    from utils.datasets import HashingDataset, OneHot, raw_collate
    from utils.transforms import _NORMS
    dev = torch.device("cuda:0")
    root = str(tmp_path)
    sizes = SIZES + [(375, 250), (256, 256), (64, 48), (333, 399)]
    _write_dataset(root, sizes, progressive_every=4)
    n = len(sizes)
    cpu = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5))
    raw = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5), gpu_preprocess=True)
    jpg = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5), gpu_decode=True)
    pre32 = GpuPreprocess(256, 224, *_NORMS[3], out_dtype=torch.float32, device=dev)
    pre16 = GpuPreprocess(256, 224, *_NORMS[3], out_dtype=torch.bfloat16, device=dev)
    dec = GpuJpegDecoder(device=dev)
    for seed in (5, 77, 901):
        torch.manual_seed(seed)
        want = torch.stack([cpu[i][0] for i in range(n)])
        torch.manual_seed(seed)
        b, _, _ = raw_collate([raw[i] for i in range(n)])
        got = pre32(b.pixels.to(dev), b.sizes, flips=b.flips, ta=b.ta).cpu()
        assert torch.equal(got, want), (seed, b.ta.tolist())
        assert torch.equal(pre16(b.pixels.to(dev), b.sizes, flips=b.flips, ta=b.ta).cpu(), want.to(torch.bfloat16))
        torch.manual_seed(seed)
        jb, _, _ = jpg[list(range(n))]
        staged = dec.host_stage(jb)
        assert torch.equal(staged.ta, b.ta) and torch.equal(staged.flips, b.flips)
        pixels, psizes = staged.finish()
        assert torch.equal(pre32(pixels, psizes, flips=staged.flips, ta=staged.ta).cpu(), want)


def test_trainer_train_loader_with_trivialaugment_sees_the_cpu_loaders_batches(tmp_path, monkeypatch):
    """COOPTrainer's own plumbing (shuffling loader -> iterate_loader -> compute_features_one_batch) with the TA list: the GPU paths hand
    the model the bf16 rounding of the CPU loader's batches, with the same images and labels."""
    import engine
    from concepthash_amd import config as cfglib
    from trainers.coop import COOPTrainer
    from utils.datasets import HashingDataset, OneHot
    monkeypatch.setattr(engine, "default_workers", 0)
    root = str(tmp_path)
    sizes = SIZES + [(300, 300), (200, 380), (390, 210), (256, 256)]
    _write_dataset(root, sizes)
    seen = {}

    class Model(torch.nn.Module):
        def forward(self, x):
            return None, {"codes": x.float().mean(dim=(1, 2, 3)).view(-1, 1)}

    for mode in ("cpu", "gpu_preprocess", "gpu_decode"):
        conf = cfglib.DictConfig(device="cuda", batch_size=4, model=cfglib.DictConfig(),
                                 dataset=cfglib.DictConfig(multiclass=False, resize=256, crop=224, norm=3))
        tr = COOPTrainer(conf)
        tr.dataset = {"test": [], "db": [], "train": HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5),
                                                                     gpu_preprocess=mode == "gpu_preprocess", gpu_decode=mode == "gpu_decode")}
        tr.load_dataloader()
        tr.model = Model()
        torch.manual_seed(2024)
        batches = []
        for data in tr.iterate_loader(tr.dataloader["train"]):
            (image, labels, index), _ = tr.compute_features_one_batch(data)
            batches.append((image.detach().to(torch.bfloat16).cpu(), labels.cpu(), index.cpu()))
        assert len(batches) == len(sizes) // 4
        seen[mode] = batches
    for mode in ("gpu_preprocess", "gpu_decode"):
        for (ia, la, xa), (ib, lb, xb) in zip(seen["cpu"], seen[mode]):
            assert torch.equal(xa, xb) and torch.equal(la, lb)
            assert torch.equal(ia, ib), mode
    # a list whose Resize / CenterCrop differ from the dataset config's geometry is refused
    conf = cfglib.DictConfig(device="cuda", batch_size=4, model=cfglib.DictConfig(),
                             dataset=cfglib.DictConfig(multiclass=False, resize=288, crop=224, norm=3))
    tr = COOPTrainer(conf)
    tr.dataset = {"test": [], "db": [], "train": HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5),
                                                                 gpu_preprocess=True)}
    tr.load_dataloader()
    tr.model = Model()
    with pytest.raises(ValueError, match="Resize"):
        for data in tr.iterate_loader(tr.dataloader["train"]):
            tr.compute_features_one_batch(data)


def test_main_v2_trains_two_epochs_with_trivialaugment(tmp_path):
    """`python main_v2.py exp=hashing dataset=cub200 transforms=trivialaugment ...` on a handful of JPEG files (gpu_decode, the default):
    two epochs finish with finite losses."""
    import json
    import math
    import os
    import subprocess
    import sys
    from conftest import ROOT
    data = tmp_path / "data" / "cub200_2011"
    data.mkdir(parents=True)
    _write_dataset(str(data), [(300, 400), (400, 300), (300, 300), (250, 330)] * 4)
    lines = open(data / "train.txt").read()
    for name in ("test.txt", "database.txt"):
        (data / name).write_text(lines)
    logdir = str(tmp_path / "run")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "dataset=cub200", "transforms=trivialaugment",
                    "dataset.nclass=5", "data_dir=" + str(tmp_path), "optim=sgd", "optim.lr=0.02", "scheduler=no_decay",
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "epochs=2", "eval_interval=0",
                    "batch_size=8", "logdir=" + logdir], check=True, env=env, cwd=str(tmp_path), timeout=600)
    tr = json.load(open(os.path.join(logdir, "train_history.json")))
    assert len(tr) == 2 and all(math.isfinite(t["train_loss"]) for t in tr), tr
