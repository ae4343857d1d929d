"""`utils.transforms` (un-vendored in the reference; call sites configs/dataset/cub200.yaml:10-47) plus the four
torchvision eval transforms those configs name -- torchvision is not installed in the target image, so
`concepthash_amd.config.locate` maps `torchvision.transforms.{Resize, CenterCrop, ToTensor, Compose}` here.

`normalize_transform(norm)`: the reference's constants live in the missing module; `norm=3` is what the ConceptHash
config selects (configs/model/concept_hash_final_v1_nosa_apt.yaml:72-73) and is taken to be the CLIP statistics
(unpinned); `norm=2` ImageNet, `norm=1` 0.5/0.5, `norm=0` identity."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

_NORMS = {
    0: ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    1: ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    2: ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    3: ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
}


def interpolation(name: str):
    return {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


class Normalize:
    def __init__(self, mean, std):
        self.mean = torch.tensor(mean).view(3, 1, 1)
        self.std = torch.tensor(std).view(3, 1, 1)

    def __call__(self, x):
        return (x - self.mean) / self.std


def normalize_transform(norm: int):
    return Normalize(*_NORMS[int(norm)])


class Resize:
    def __init__(self, size, interpolation=Image.BILINEAR):
        self.size, self.interp = size, interpolation

    def __call__(self, img):
        if isinstance(self.size, int):          # shorter side -> size, aspect kept; the long side TRUNCATES, as
            w, h = img.size                     # torchvision's _compute_resized_output_size does: int(size * long / short)
            if w <= h:
                nw, nh = self.size, max(1, int(self.size * h / w))
            else:
                nw, nh = max(1, int(self.size * w / h)), self.size
            return img.resize((nw, nh), self.interp)
        return img.resize((self.size[1], self.size[0]), self.interp)


class CenterCrop:
    def __init__(self, size):
        self.size = (size, size) if isinstance(size, int) else tuple(size)

    def __call__(self, img):
        w, h = img.size
        th, tw = self.size
        left, top = int(round((w - tw) / 2.0)), int(round((h - th) / 2.0))
        return img.crop((left, top, left + tw, top + th))


class ToTensor:
    def __call__(self, img):
        a = np.array(img.convert("RGB"), dtype=np.uint8)      # a writable copy: torch.from_numpy warns about PIL's read-only buffer
        return torch.from_numpy(a).permute(2, 0, 1).float().div_(255.0)


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class RandomResizedCrop:
    """torchvision.transforms.RandomResizedCrop as the reference's train_dataset uses it (configs/dataset/cub200.yaml:13-19):
    area fraction U(0.08, 1), log-uniform aspect ratio in (3/4, 4/3), ten tries, then the centre-crop fallback."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation=Image.BILINEAR):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.scale, self.ratio, self.interp = tuple(scale), tuple(ratio), interpolation

    def get_params(self, w, h):
        import math
        area = w * h
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = area * float(torch.empty(1).uniform_(self.scale[0], self.scale[1]))
            ar = math.exp(float(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])))
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                top = int(torch.randint(0, h - ch + 1, (1,)))
                left = int(torch.randint(0, w - cw + 1, (1,)))
                return top, left, ch, cw
        in_ratio = w / h
        if in_ratio < self.ratio[0]:
            cw, ch = w, int(round(w / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            ch, cw = h, int(round(h * self.ratio[1]))
        else:
            cw, ch = w, h
        return (h - ch) // 2, (w - cw) // 2, ch, cw

    def __call__(self, img):
        w, h = img.size
        top, left, ch, cw = self.get_params(w, h)
        return img.crop((left, top, left + cw, top + ch)).resize((self.size[1], self.size[0]), self.interp)


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img):
        return img.transpose(Image.FLIP_LEFT_RIGHT) if float(torch.rand(1)) < self.p else img


# ---------------------------------------------------------------------------------------------------------------------------------
# TrivialAugmentWide (torchvision >= 0.13, v1 API) as the reference's configs/transforms/trivialaugment.yaml uses it.  The random
# draws (`draw`) and the PIL arithmetic (`apply`) are split so that a GPU-path loader makes exactly these random calls and the host
# planner derives the same per-image parameters (`op_params`) that `apply` hands Pillow.
# ---------------------------------------------------------------------------------------------------------------------------------
TA_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
          "Posterize", "Solarize", "AutoContrast", "Equalize")


def ta_augmentation_space(num_bins: int = 31):
    """op name -> (magnitudes, signed): torchvision's TrivialAugmentWide._augmentation_space, float32 torch tensors."""
    return {
        "Identity": (torch.tensor(0.0), False),
        "ShearX": (torch.linspace(0.0, 0.99, num_bins), True),
        "ShearY": (torch.linspace(0.0, 0.99, num_bins), True),
        "TranslateX": (torch.linspace(0.0, 32.0, num_bins), True),
        "TranslateY": (torch.linspace(0.0, 32.0, num_bins), True),
        "Rotate": (torch.linspace(0.0, 135.0, num_bins), True),
        "Brightness": (torch.linspace(0.0, 0.99, num_bins), True),
        "Color": (torch.linspace(0.0, 0.99, num_bins), True),
        "Contrast": (torch.linspace(0.0, 0.99, num_bins), True),
        "Sharpness": (torch.linspace(0.0, 0.99, num_bins), True),
        "Posterize": (8 - (torch.arange(num_bins) / ((num_bins - 1) / 6)).round().int(), False),
        "Solarize": (torch.linspace(255.0, 0.0, num_bins), False),
        "AutoContrast": (torch.tensor(0.0), False),
        "Equalize": (torch.tensor(0.0), False),
    }


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix (inverted=True), Python doubles."""
    import math
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_plan(angle, w, h):
    """What Pillow's Image.rotate(angle, expand=False) does to a w x h image: ("copy", None), ("transpose", ROTATE_90 / ROTATE_270) or
    ("affine", the 6 doubles it hands Image.transform) -- its own fast paths and its matrix, restated."""
    import math
    angle = angle % 360.0
    if angle == 0:
        return "copy", None
    if angle == 180:
        return "transpose", Image.Transpose.ROTATE_180
    if angle in (90, 270) and w == h:
        return "transpose", Image.Transpose.ROTATE_90 if angle == 90 else Image.Transpose.ROTATE_270
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return "affine", m


def ta_op_params(op: int, m: float, w: int, h: int):
    """(kind, value) of TrivialAugmentWide op `op` with signed magnitude `m` on a w x h image, as `TrivialAugmentWide.apply` hands them to
    Pillow: ("affine", M) for the geometric ops (the inverse matrix of torchvision's PIL branch of F.affine, or Pillow's rotate matrix),
    ("copy" | "transpose", ...) for rotate's fast paths, ("blend", 1 + m) for the four enhancers, ("bits", int(m)), ("threshold", m),
    ("none", None) for Identity / AutoContrast / Equalize."""
    import math
    name = TA_OPS[op]
    if name == "ShearX":
        return "affine", inverse_affine_matrix([0, 0], 0.0, [0, 0], 1.0, [math.degrees(math.atan(m)), 0.0])
    if name == "ShearY":
        return "affine", inverse_affine_matrix([0, 0], 0.0, [0, 0], 1.0, [0.0, math.degrees(math.atan(m))])
    if name == "TranslateX":
        return "affine", inverse_affine_matrix([w * 0.5, h * 0.5], 0.0, [int(m), 0], 1.0, [0.0, 0.0])
    if name == "TranslateY":
        return "affine", inverse_affine_matrix([w * 0.5, h * 0.5], 0.0, [0, int(m)], 1.0, [0.0, 0.0])
    if name == "Rotate":
        return rotate_plan(m, w, h)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return "blend", 1.0 + m
    if name == "Posterize":
        return "bits", int(m)
    if name == "Solarize":
        return "threshold", m
    return "none", None


class TrivialAugmentWide:
    """torchvision.transforms.TrivialAugmentWide on PIL images: one op of `TA_OPS` drawn uniformly, one of `num_magnitude_bins`
    magnitudes, a random sign for the signed ops; Pillow does the arithmetic (`apply`).  `fill=None` is black, as torchvision's
    _parse_fill makes it."""

    def __init__(self, num_magnitude_bins: int = 31, interpolation=Image.NEAREST, fill=None):
        self.num_magnitude_bins = int(num_magnitude_bins)
        self.interpolation = interpolation
        self.fill = fill
        self.space = ta_augmentation_space(self.num_magnitude_bins)

    def draw(self):
        """(op index, signed magnitude): torchvision's random calls, in its order."""
        op = int(torch.randint(len(TA_OPS), (1,)).item())
        mags, signed = self.space[TA_OPS[op]]
        m = float(mags[torch.randint(len(mags), (1,), dtype=torch.long)].item()) if mags.ndim > 0 else 0.0
        if signed and torch.randint(2, (1,)):
            m *= -1.0
        return op, m

    def _fillcolor(self, img):
        fill = 0 if self.fill is None else self.fill
        if isinstance(fill, (int, float)) and len(img.getbands()) > 1:
            return tuple([fill] * len(img.getbands()))
        return tuple(fill) if isinstance(fill, (list, tuple)) else fill

    def apply(self, img, op: int, m: float):
        from PIL import ImageEnhance, ImageOps
        name = TA_OPS[op]
        fillcolor = self._fillcolor(img)
        if name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
            M = ta_op_params(op, m, *img.size)[1]
            return img.transform(img.size, Image.AFFINE, M, self.interpolation, fillcolor=fillcolor)
        if name == "Rotate":
            return img.rotate(m, self.interpolation, expand=False, fillcolor=fillcolor)
        if name == "Brightness":
            return ImageEnhance.Brightness(img).enhance(1.0 + m)
        if name == "Color":
            return ImageEnhance.Color(img).enhance(1.0 + m)
        if name == "Contrast":
            return ImageEnhance.Contrast(img).enhance(1.0 + m)
        if name == "Sharpness":
            return ImageEnhance.Sharpness(img).enhance(1.0 + m)
        if name == "Posterize":
            return ImageOps.posterize(img, int(m))
        if name == "Solarize":
            return ImageOps.solarize(img, m)
        if name == "AutoContrast":
            return ImageOps.autocontrast(img)
        if name == "Equalize":
            return ImageOps.equalize(img)
        return img

    def __call__(self, img):
        return self.apply(img, *self.draw())
