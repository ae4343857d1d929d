"""TrivialAugmentWide (the reference's configs/transforms/trivialaugment.yaml), CPU side: the config group, the op table and the
random calls of torchvision's TrivialAugmentWide, each op against the direct Pillow call, the loader's draws on the GPU paths, and a
numpy restatement of the Pillow C arithmetic that csrc/augment.hip ports (blend, RGB -> L, SMOOTH, the bicubic affine sampler),
pinned against the installed Pillow."""
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

from test_preprocess import _image, _write_dataset


def _ta_chain(interpolation="bicubic", fill=None, norm=3):
    from utils import transforms as T
    return [T.Resize(256), T.RandomHorizontalFlip(), T.TrivialAugmentWide(interpolation=T.interpolation(interpolation), fill=fill),
            T.CenterCrop(224), T.ToTensor(), T.normalize_transform(norm)]


def test_transforms_group_composes_the_reference_chain_over_the_dataset():
    import os
    from concepthash_amd import config as C
    from utils import transforms as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.compose(os.path.join(root, "configs"), "train", ["dataset=cub200", "transforms=trivialaugment"])
    ts = cfg.dataset.train_dataset.transform
    assert [t["_target_"] for t in ts] == ["torchvision.transforms.Resize", "torchvision.transforms.RandomHorizontalFlip",
                                           "torchvision.transforms.TrivialAugmentWide", "torchvision.transforms.CenterCrop",
                                           "torchvision.transforms.ToTensor", "utils.transforms.normalize_transform"]
    assert ts[0]["size"] == cfg.dataset.resize == 256 and ts[3]["size"] == cfg.dataset.crop == 224
    assert ts[5]["norm"] == cfg.dataset.norm == 3                   # the model file's norm, applied before the transform group
    objs = [C.instantiate(t) for t in ts]
    assert isinstance(objs[2], T.TrivialAugmentWide) and objs[2].interpolation == Image.BICUBIC and objs[2].fill is None
    assert C.locate("torchvision.transforms.TrivialAugmentWide") is T.TrivialAugmentWide
    # the default composition is untouched: the dataset file's RandomResizedCrop list
    plain = C.compose(os.path.join(root, "configs"), "train", ["dataset=cub200"])
    assert plain.dataset.train_dataset.transform[0]["_target_"] == "torchvision.transforms.RandomResizedCrop"
    # a synthetic dataset has no images to apply a selected list to: it says so instead of ignoring it
    syn = C.compose(os.path.join(root, "configs"), "train", ["dataset=synthetic_cub200", "transforms=trivialaugment"])
    with pytest.raises(ValueError, match="transform"):
        C.instantiate(syn.dataset.train_dataset)


def test_op_table_is_torchvisions():
    from utils.transforms import TA_OPS, ta_augmentation_space
    space = ta_augmentation_space(31)
    assert list(space) == list(TA_OPS) and len(TA_OPS) == 14
    f = torch.linspace(0.0, 0.99, 31)
    want = {"ShearX": f, "ShearY": f, "TranslateX": torch.linspace(0.0, 32.0, 31), "TranslateY": torch.linspace(0.0, 32.0, 31),
            "Rotate": torch.linspace(0.0, 135.0, 31), "Brightness": f, "Color": f, "Contrast": f, "Sharpness": f,
            "Posterize": 8 - (torch.arange(31) / ((31 - 1) / 6)).round().int(), "Solarize": torch.linspace(255.0, 0.0, 31)}
    for name, (mags, signed) in space.items():
        if name in want:
            assert mags.dtype == want[name].dtype and torch.equal(mags, want[name]), name
            assert signed == (name not in ("Posterize", "Solarize"))
        else:
            assert mags.ndim == 0 and float(mags) == 0.0 and not signed
    assert space["Posterize"][0].tolist()[:4] == [8, 8, 8, 7] and float(space["Rotate"][0][20]) == 90.0


def _hand_draws(n, seed):
    """torchvision's random calls written out: op, then (non-0-dim magnitudes) the bin, then (signed ops) the sign"""
    from utils.transforms import TA_OPS, ta_augmentation_space
    space = ta_augmentation_space(31)
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        op = int(torch.randint(14, (1,)))
        mags, signed = space[TA_OPS[op]]
        m = float(mags[torch.randint(len(mags), (1,), dtype=torch.long)].item()) if mags.ndim else 0.0
        if signed and bool(torch.randint(2, (1,))):
            m = -m
        out.append((op, m))
    return out, torch.rand(1)


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
def test_draws_are_torchvisions_random_calls(seed):
    from utils.transforms import TrivialAugmentWide
    want, after = _hand_draws(200, seed)
    ta = TrivialAugmentWide()
    torch.manual_seed(seed)
    got = [ta.draw() for _ in range(200)]
    assert got == want and torch.equal(torch.rand(1), after)       # the same number of calls: the stream stays in step
    assert {op for op, _ in got} == set(range(14))
    for op, m in got:
        if op in (0, 12, 13):
            assert m == 0.0


def test_magnitude_free_and_unsigned_ops_make_no_extra_draws():
    from utils.transforms import TrivialAugmentWide
    ta = TrivialAugmentWide()
    for op, ncalls in ((0, 1), (12, 1), (13, 1), (10, 2), (11, 2), (1, 3), (6, 3)):
        # force the op: find a seed whose first randint(14) is `op`, then count the calls by comparing the stream afterwards
        for seed in range(2000):
            torch.manual_seed(seed)
            if int(torch.randint(14, (1,))) == op:
                break
        torch.manual_seed(seed)
        ta.draw()
        nxt = torch.randint(1 << 30, (1,))
        torch.manual_seed(seed)
        for _ in range(ncalls):
            torch.randint(2, (1,))
        assert torch.equal(torch.randint(1 << 30, (1,)), nxt), (op, ncalls)


@pytest.mark.parametrize("op", range(14))
def test_each_op_is_the_direct_pillow_call(op):
    from utils.transforms import TrivialAugmentWide, ta_op_params
    ta = TrivialAugmentWide(interpolation=Image.BICUBIC)
    for (h, w), m in (((40, 56), 0.5), ((56, 40), -0.33), ((48, 48), 90.0), ((48, 48), -90.0), ((31, 45), 13.0), ((45, 31), -27.2)):
        img = Image.fromarray(_image(h, w, op))
        mm = {10: 5.0, 11: 120.5}.get(op, m)
        got = np.asarray(ta.apply(img, op, mm))
        M = None
        if op == 1:
            M = [1, math.tan(math.atan(mm)), 0, 0, 1, 0]
            ref = img.transform(img.size, Image.AFFINE, ta_op_params(op, mm, w, h)[1], Image.BICUBIC, fillcolor=(0, 0, 0))
            assert np.allclose(ta_op_params(op, mm, w, h)[1], M)            # x' = x + tan(shear) * y about [0, 0]
        elif op == 2:
            ref = img.transform(img.size, Image.AFFINE, ta_op_params(op, mm, w, h)[1], Image.BICUBIC, fillcolor=(0, 0, 0))
            assert np.allclose(ta_op_params(op, mm, w, h)[1], [1, 0, 0, math.tan(math.atan(mm)), 1, 0])
        elif op in (3, 4):
            ref = img.transform(img.size, Image.AFFINE, ta_op_params(op, mm, w, h)[1], Image.BICUBIC, fillcolor=(0, 0, 0))
            t = float(int(mm))
            assert np.allclose(ta_op_params(op, mm, w, h)[1], [1, 0, -t, 0, 1, 0] if op == 3 else [1, 0, 0, 0, 1, -t])
        elif op == 5:
            ref = img.rotate(mm, Image.BICUBIC, expand=False, fillcolor=(0, 0, 0))
        elif op in (6, 7, 8, 9):
            enh = (ImageEnhance.Brightness, ImageEnhance.Color, ImageEnhance.Contrast, ImageEnhance.Sharpness)[op - 6]
            ref = enh(img).enhance(1.0 + mm)
        elif op == 10:
            ref = ImageOps.posterize(img, 5)
        elif op == 11:
            ref = ImageOps.solarize(img, 120.5)
        elif op == 12:
            ref = ImageOps.autocontrast(img)
        elif op == 13:
            ref = ImageOps.equalize(img)
        else:
            ref = img
        assert np.array_equal(got, np.asarray(ref)), (op, h, w, mm)


def test_rotate_plan_is_pillows_rotate():
    """the host planner's restatement of Image.rotate: the fast paths it takes, and the matrix otherwise"""
    from utils.transforms import rotate_plan
    for (h, w) in ((48, 48), (40, 56)):
        img = Image.fromarray(_image(h, w, 3))
        for angle in (0.0, -0.0, 4.5, -4.5, 90.0, -90.0, 130.5, -135.0):
            kind, val = rotate_plan(angle, w, h)
            ref = np.asarray(img.rotate(angle, Image.BICUBIC, expand=False, fillcolor=(0, 0, 0)))
            if kind == "copy":
                got = np.asarray(img)
            elif kind == "transpose":
                assert w == h and abs(angle) == 90.0
                got = np.asarray(img.transpose(val))
                assert np.array_equal(got, np.rot90(np.asarray(img), 1 if angle % 360 == 90 else -1))
            else:
                got = np.asarray(img.transform(img.size, Image.AFFINE, val, Image.BICUBIC, fillcolor=(0, 0, 0)))
            assert np.array_equal(got, ref), (h, w, angle, kind)


# ---- numpy restatement of the Pillow C arithmetic that csrc/augment.hip ports -------------------------------------------------

def _to_l(a):
    a = a.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def _blend(deg, img, alpha):
    al = np.float32(alpha)
    d = deg.astype(np.int32)
    v = d.astype(np.float32) + al * (img.astype(np.int32) - d).astype(np.float32)
    if 0.0 <= al <= 1.0:
        return v.astype(np.int32).astype(np.uint8)
    return np.where(v <= 0, 0, np.where(v >= 255, 255, v)).astype(np.int32).astype(np.uint8)


def _smooth(a):
    out = a.copy()
    h, w, _ = a.shape
    f = a.astype(np.float32)
    k1, k5 = np.float32(1.0 / 13.0), np.float32(5.0 / 13.0)
    s = np.full((h - 2, w - 2, 3), 0.5, np.float32)
    for dy in (1, 0, -1):
        r = f[1 + dy:h - 1 + dy]
        s = s + ((r[:, 0:w - 2] * k1 + r[:, 1:w - 1] * (k5 if dy == 0 else k1)) + r[:, 2:w] * k1)
    out[1:-1, 1:-1] = np.where(s <= 0, 0, np.where(s >= 255, 255, s)).astype(np.int32).astype(np.uint8)
    return out


def _cubic(v1, v2, v3, v4, d):
    p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _affine(a, M):
    h, w, _ = a.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xin = M[0] * (xx + 0.5) + M[1] * (yy + 0.5) + M[2]
    yin = M[3] * (xx + 0.5) + M[4] * (yy + 0.5) + M[5]
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - x, yin - y
    x, y = x - 1, y - 1
    xs = [np.clip(x + k, 0, w - 1) for k in range(4)]
    out = np.zeros_like(a)
    for b in range(3):
        ch = a[..., b].astype(np.float64)
        rows = [np.clip(y, 0, h - 1)]
        vals = [_cubic(*[ch[rows[0], xk] for xk in xs], dx)]
        for k in (1, 2, 3):
            ok = (y + k >= 0) & (y + k < h)
            r = np.clip(y + k, 0, h - 1)
            vals.append(np.where(ok, _cubic(*[ch[r, xk] for xk in xs], dx), vals[-1]))
        v = _cubic(*vals, dy)
        out[..., b] = np.where(inside, np.where(v <= 0, 0, np.where(v >= 255, 255, v)), 0).astype(np.int32).astype(np.uint8)
    return out


def test_numpy_restatement_of_pillows_c_arithmetic():
    from utils.transforms import ta_op_params
    rng = np.random.default_rng(0)
    for it in range(12):
        h, w = int(rng.integers(5, 48)), int(rng.integers(5, 48))
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if it % 3 == 0:
            a = (a // 61 * 61).astype(np.uint8)                        # flat areas: ties in the float sums
        img = Image.fromarray(a)
        assert np.array_equal(_to_l(a), np.asarray(img.convert("L")))
        assert np.array_equal(_smooth(a), np.asarray(img.filter(ImageFilter.SMOOTH)))
        L = np.repeat(_to_l(a)[..., None], 3, 2)
        for f in (0.01, 0.37, 0.967, 1.0, 1.033, 1.5, 1.99):
            assert np.array_equal(_blend(np.zeros_like(a), a, f), np.asarray(ImageEnhance.Brightness(img).enhance(f))), f
            assert np.array_equal(_blend(L, a, f), np.asarray(ImageEnhance.Color(img).enhance(f))), f
            assert np.array_equal(_blend(_smooth(a), a, f), np.asarray(ImageEnhance.Sharpness(img).enhance(f))), f
        for op, m in ((1, 0.3), (1, -0.99), (2, 0.66), (3, 13.0), (4, -32.0), (5, 47.25), (5, -130.5), (5, 4.5)):
            kind, M = ta_op_params(op, m, w, h)
            assert kind == "affine"
            ref = np.asarray(img.transform(img.size, Image.AFFINE, M, Image.BICUBIC, fillcolor=(0, 0, 0)))
            assert np.array_equal(_affine(a, M), ref), (op, m)


# ---- the loader side ---------------------------------------------------------------------------------------------------------

def test_gpu_augmentation_accepts_the_ta_list_and_refuses_other_arrangements():
    from utils import transforms as T
    from utils.datasets import TrivialAugmentChain, gpu_augmentation
    chain = gpu_augmentation(T.Compose(_ta_chain()))
    assert isinstance(chain, TrivialAugmentChain) and (chain.resize, chain.crop) == (256, 224) and chain.flip is not None
    no_flip = [t for t in _ta_chain() if not isinstance(t, T.RandomHorizontalFlip)]
    assert gpu_augmentation(no_flip).flip is None
    bad = [_ta_chain(fill=0), _ta_chain(fill=(1, 2, 3)), _ta_chain(interpolation="nearest"), _ta_chain(interpolation="bilinear")]
    after_crop = _ta_chain()
    after_crop[2], after_crop[3] = after_crop[3], after_crop[2]
    bad.append(after_crop)
    bad.append([T.Resize(256, T.interpolation("bicubic"))] + _ta_chain()[1:])            # Resize must be torchvision's default bilinear
    bad.append([T.RandomResizedCrop(224, interpolation=T.interpolation("bicubic")), T.TrivialAugmentWide(interpolation=Image.BICUBIC),
                T.ToTensor()])
    bad.append(_ta_chain()[:3] + [T.CenterCrop((224, 200))] + _ta_chain()[4:])
    for lst in bad:
        with pytest.raises(ValueError):
            gpu_augmentation(lst)
    # lists without TrivialAugmentWide keep their handling
    assert gpu_augmentation([T.Resize(256, T.interpolation("bicubic")), T.CenterCrop(224), T.ToTensor()]) is None
    assert gpu_augmentation([T.RandomResizedCrop(224, interpolation=T.interpolation("bicubic")), T.ToTensor()])[1] is None


def test_loader_draws_are_the_cpu_chains(tmp_path):
    """The worker of a GPU-path dataset with the TA list makes the CPU chain's random calls in its order: flip, then op / magnitude /
    sign.  The draws, applied through the PIL chain by hand, give the CPU dataset's tensors."""
    from utils import transforms as T
    from utils.datasets import HashingDataset, OneHot, raw_collate
    root = str(tmp_path)
    sizes = [(60, 80), (90, 70), (64, 64), (33, 50), (120, 90), (70, 70)]
    _write_dataset(root, sizes)
    n = len(sizes)
    cpu = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5))
    raw = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5), gpu_preprocess=True)
    jpg = HashingDataset(root, "train.txt", transform=_ta_chain(), target_transform=OneHot(5), gpu_decode=True)
    for seed in (3, 11):
        torch.manual_seed(seed)
        want = [cpu[i][0] for i in range(n)]
        torch.manual_seed(seed)
        b, _, _ = raw_collate([raw[i] for i in range(n)])
        torch.manual_seed(seed)
        jb, _, _ = jpg[list(range(n))]
        torch.manual_seed(seed)
        single = [jpg[i][0] for i in range(n)]
        assert b.boxes is None and b.ta.shape == (n, 2) and b.ta.dtype == torch.float64
        assert torch.equal(jb.ta, b.ta) and torch.equal(jb.flips, b.flips) and jb.boxes is None
        assert all(tuple(single[i][3]) == tuple(b.ta[i].tolist()) and single[i][2] == bool(b.flips[i]) for i in range(n))
        ta = T.TrivialAugmentWide(interpolation=Image.BICUBIC)
        offs = np.cumsum([0] + [h * w * 3 for h, w in b.sizes])
        for i, (h, w) in enumerate(b.sizes):
            img = Image.fromarray(b.pixels[offs[i]:offs[i + 1]].view(h, w, 3).numpy())
            img = T.Resize(256)(img)
            if bool(b.flips[i]):
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            img = ta.apply(img, int(b.ta[i, 0]), float(b.ta[i, 1]))
            x = T.normalize_transform(3)(T.ToTensor()(T.CenterCrop(224)(img)))
            assert torch.equal(x, want[i]), i


def test_host_plan_carries_the_op_scalars():
    """GpuPreprocess.plan_augment's descriptors (no GPU needed for the plan): geometry of Resize(256, bilinear) -> CenterCrop(224), the
    flip, and per op the scalars TrivialAugmentWide.apply hands Pillow."""
    from concepthash_amd.preprocess import GpuPreprocess, _row_bounds_bilinear
    from utils.transforms import rotate_plan
    pre = GpuPreprocess.__new__(GpuPreprocess)
    from concepthash_amd import _lib
    pre.lib, pre.resize, pre.crop, pre.max_taps = _lib.load(), 256, 224, 64
    sizes = [(375, 500), (500, 375), (300, 300), (30, 40), (300, 300), (375, 500), (375, 500), (375, 500), (9000, 8000)]
    ta = [(1, 0.33), (3, -21.0), (5, 90.0), (6, -0.5), (5, 0.0), (10, 4.0), (11, 127.5), (5, 30.0), (0, 0.0)]
    flips = [True, False, True, False, False, True, False, False, False]
    desc, nbytes, ws, max_rows, max_nh, max_nw = pre.plan_augment(sizes, flips, ta)
    assert nbytes == sum(h * w * 3 for h, w in sizes)
    assert tuple(desc[0][["nh", "nw", "top", "left", "flip", "op"]]) == (256, 341, 16, 58, 1, 1)
    assert np.allclose(desc["m"][0], [1, 0.33, 0, 0, 1, 0]) and desc["row0"][0] == 0 and desc["nrows"][0] == 375
    assert np.allclose(desc["m"][1], [1, 0, 21, 0, 1, 0])
    assert desc["iparam"][2] == 2 and desc["iparam"][4] == 1                 # square +90: ROTATE_90; 0: copy
    assert desc["fparam"][3] == 0.5 and desc["iparam"][5] == 4 and desc["fparam"][6] == 127.5
    assert list(desc["m"][7]) == rotate_plan(30.0, 341, 256)[1]
    assert desc["nrows"][8] == 0 and max_nh == 341 and max_nw == 341          # past the tap limit: the host route
    assert _row_bounds_bilinear(30, 256, 0)[0] == 0 and sum(_row_bounds_bilinear(30, 256, 255)) == 30
    ends = desc["img_offset"][:8] + desc["nh"][:8].astype(np.int64) * desc["nw"][:8] * 3
    assert int(ends.max()) == ws and (desc["tmp_offset"][:8] >= int(pre.lib.ch_augment_workspace(len(sizes), 0))).all()
