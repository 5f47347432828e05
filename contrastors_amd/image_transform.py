"""Image transform of the image-text data path (sc/dataset/transform.py:23-119 `image_transform`): the reference runs
`RandomResizedCrop(S, scale, BICUBIC)` (train) or `Resize(S, BICUBIC)` + `CenterCrop(S)` (eval), `ToTensor` and `Normalize`
with torchvision on PIL images in the loader workers.  Here the workers only decode; crop, resize, normalize, layout and
dtype are one HIP kernel (csrc/image.hip, `cx_image_transform`) over a ragged batch of decoded images.

Host side (pure functions, no GPU):
  * random_resized_crop_params  torchvision's `RandomResizedCrop.get_params`, drawn from a torch.Generator
  * train_plan / eval_plan      the per-image plan the kernel takes: clamp ranges (y_lo, y_hi, x_lo, x_hi) int32 and
                                (y_origin, y_scale, x_origin, x_scale) float64
GpuImageTransform turns {"pixels_u8", "offsets", "sizes"} into the (B, 3, S, S) tensor `ViTEngine` takes.
"""
from __future__ import annotations

import logging
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

OPENAI_DATASET_MEAN = (0.48145466, 0.4578275, 0.40821073)   # sc/constants.py (TransformsConfig defaults)
OPENAI_DATASET_STD = (0.26862954, 0.26130258, 0.27577711)

# what cx_image_transform serves (include/contrastors_hip.h)
MAX_SIDE, MAX_SCALE, MAX_IMAGE_SIZE = 8192, 16.0, 512

log = logging.getLogger(__name__)


def random_resized_crop_params(h: int, w: int, scale: Sequence[float] = (0.9, 1.0), ratio: Sequence[float] = (3 / 4, 4 / 3),
                               generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int]:
    """(top, left, crop_h, crop_w) as torchvision's RandomResizedCrop.get_params draws it: up to 10 tries of an area and a
    log-uniform aspect ratio, then the central crop with the aspect ratio clamped to `ratio`."""
    area = h * w
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = math.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator).item())
        cw = int(round(math.sqrt(target_area * aspect)))
        ch = int(round(math.sqrt(target_area / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            top = int(torch.randint(0, h - ch + 1, (1,), generator=generator).item())
            left = int(torch.randint(0, w - cw + 1, (1,), generator=generator).item())
            return top, left, ch, cw
    in_ratio = w / h
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def train_plan(box: Sequence[int], S: int):
    """Integer crop (top, left, ch, cw), then resize to (S, S): torchvision crops first, so the taps never leave the crop."""
    top, left, ch, cw = (int(v) for v in box)
    return (top, top + ch, left, left + cw), (float(top), ch / S, float(left), cw / S)


def eval_plan(h: int, w: int, S: int):
    """Resize(S) (shorter side -> S, longer -> int(S * long / short)) then CenterCrop(S), as one plan over the whole image."""
    if w <= h:
        new_w, new_h = S, int(S * h / w)
    else:
        new_h, new_w = S, int(S * w / h)
    off_y, off_x = int(round((new_h - S) / 2.0)), int(round((new_w - S) / 2.0))
    y_scale, x_scale = h / new_h, w / new_w
    return (0, h, 0, w), (off_y * y_scale, y_scale, off_x * x_scale, x_scale)


def host_resize(img: np.ndarray, plan_i, plan_f, S: int) -> np.ndarray:
    """One image resized to its plan with PIL: crop to the clamp range, then BICUBIC resize of the plan's box -> (S, S, 3) uint8."""
    from PIL import Image

    y_lo, y_hi, x_lo, x_hi = (int(v) for v in plan_i)
    y_origin, y_scale, x_origin, x_scale = (float(v) for v in plan_f)
    crop = Image.fromarray(np.ascontiguousarray(img[y_lo:y_hi, x_lo:x_hi]))
    x0, y0 = max(x_origin - x_lo, 0.0), max(y_origin - y_lo, 0.0)
    x1, y1 = min(x0 + S * x_scale, float(x_hi - x_lo)), min(y0 + S * y_scale, float(y_hi - y_lo))
    return np.asarray(crop.resize((S, S), Image.BICUBIC, box=(x0, y0, x1, y1)), dtype=np.uint8)


class GpuImageTransform:
    """`image_transform(**TransformsConfig)` of the reference on the GPU.  Call it with the `vision` part of a ragged batch
    (`pixels_u8`: all images HWC uint8 back to back, `offsets`: (B + 1) int64 byte offsets, `sizes`: (B, 2) int32 rows, columns);
    it returns the (B, 3, S, S) device tensor.  Train mode draws one crop box per image from `generator` (in the calling
    process: the number of loader workers does not change them); `plans=(plan_i, plan_f)` overrides the mode's own plans."""

    def __init__(self, image_size: int = 224, mean=None, std=None, is_train: bool = True, scale=(0.9, 1.0),
                 out_dtype=torch.bfloat16, resize_longest_max: bool = False, seed: int = 0, device=None):
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise NotImplementedError(f"image_size {image_size}: square outputs only")
            image_size = image_size[0]
        if resize_longest_max:
            raise NotImplementedError("transforms.resize_longest_max (ResizeMaxSize + pad) is not served")
        if not 1 <= int(image_size) <= MAX_IMAGE_SIZE:
            raise ValueError(f"image_size must be in 1..{MAX_IMAGE_SIZE}, got {image_size}")
        if out_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"out_dtype must be torch.bfloat16 or torch.float32, got {out_dtype}")
        self.image_size, self.is_train, self.scale, self.out_dtype = int(image_size), bool(is_train), tuple(scale), out_dtype
        mean = OPENAI_DATASET_MEAN if mean is None else mean
        std = OPENAI_DATASET_STD if std is None else std
        self.mean = np.asarray((mean,) * 3 if isinstance(mean, (int, float)) else mean, np.float32)
        self.std = np.asarray((std,) * 3 if isinstance(std, (int, float)) else std, np.float32)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.device = device
        self.host_fallbacks = 0
        self._warned = False
        self._inflight = []   # (event, pinned plan tensors): the kernel reads them until the event has completed

    @classmethod
    def from_config(cls, transforms, is_train: bool, out_dtype=torch.bfloat16, seed: int = 0, device=None):
        """From a `TransformsConfig` (None = the reference's defaults).  Of aug_cfg only `scale` is honoured, as in the
        reference (sc/dataset/transform.py:60-66 reads nothing else; the colour-jitter / flip lines are commented out)."""
        if transforms is None:
            return cls(is_train=is_train, out_dtype=out_dtype, seed=seed, device=device)
        aug = dict(transforms.aug_cfg or {})
        scale = tuple(aug.pop("scale", None) or (0.9, 1.0))
        if aug and is_train:
            log.warning("transforms.aug_cfg keys %s are not used (only `scale` is, as in the reference)", sorted(aug))
        return cls(image_size=transforms.image_size, mean=transforms.mean, std=transforms.std, is_train=is_train, scale=scale,
                   out_dtype=out_dtype, resize_longest_max=transforms.resize_longest_max, seed=seed, device=device)

    def plans(self, sizes) -> Tuple[np.ndarray, np.ndarray]:
        """(B, 4) int32 and (B, 4) float64 plans of this mode for images of `sizes` (B, 2); train mode advances the generator."""
        sizes = np.asarray(sizes).reshape(-1, 2)
        plan_i, plan_f = np.empty((len(sizes), 4), np.int32), np.empty((len(sizes), 4), np.float64)
        for b, (h, w) in enumerate(sizes.tolist()):
            if self.is_train:
                box = random_resized_crop_params(h, w, self.scale, generator=self.generator)
                plan_i[b], plan_f[b] = train_plan(box, self.image_size)
            else:
                plan_i[b], plan_f[b] = eval_plan(h, w, self.image_size)
        return plan_i, plan_f

    def _host_fallback(self, pixels, offsets, sizes, plan_i, plan_f, bad):
        """Resize the images the kernel does not serve with PIL and rebuild the ragged batch around them."""
        S = self.image_size
        if not self._warned:
            log.warning("image transform: an image outside the kernel's range (side > %d or scale > %g) is resized on the host; "
                        "counted in GpuImageTransform.host_fallbacks", MAX_SIDE, MAX_SCALE)
            self._warned = True
        self.host_fallbacks += len(bad)
        parts, new_sizes, plan_i, plan_f = [], sizes.copy(), plan_i.copy(), plan_f.copy()
        for b in range(len(sizes)):
            h, w = int(sizes[b, 0]), int(sizes[b, 1])
            img = pixels[int(offsets[b]): int(offsets[b]) + 3 * h * w]
            if b in bad:
                img = host_resize(img.reshape(h, w, 3), plan_i[b], plan_f[b], S).reshape(-1)
                new_sizes[b] = (S, S)
                plan_i[b], plan_f[b] = (0, S, 0, S), (0.0, 1.0, 0.0, 1.0)
            parts.append(img)
        new_offsets = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum([p.size for p in parts], out=new_offsets[1:])
        return np.concatenate(parts), new_offsets, new_sizes, plan_i, plan_f

    def __call__(self, vision: dict, plans=None) -> torch.Tensor:
        from . import _C

        pixels, offsets, sizes = vision["pixels_u8"], vision["offsets"], vision["sizes"]
        sizes_np = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
        offsets_np = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        B, S = len(sizes_np), self.image_size
        if B == 0 or len(offsets_np) != B + 1:
            raise ValueError(f"ragged batch: {B} sizes, {len(offsets_np)} offsets (need B + 1)")
        plan_i, plan_f = plans if plans is not None else self.plans(sizes_np)
        plan_i = np.ascontiguousarray(np.asarray(plan_i, np.int32).reshape(B, 4))
        plan_f = np.ascontiguousarray(np.asarray(plan_f, np.float64).reshape(B, 4))
        bad = set(np.nonzero((sizes_np.max(1) > MAX_SIDE) | (plan_f[:, 1] > MAX_SCALE) | (plan_f[:, 3] > MAX_SCALE))[0].tolist())
        if bad:
            pix_np = pixels.cpu().numpy() if torch.is_tensor(pixels) else np.asarray(pixels, np.uint8)
            pix_np, offsets_np, sizes_np, plan_i, plan_f = self._host_fallback(pix_np, offsets_np, sizes_np, plan_i, plan_f, bad)
            pixels = torch.from_numpy(pix_np)
        if not torch.is_tensor(pixels):
            pixels = torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.uint8))
        device = self.device or torch.device("cuda", torch.cuda.current_device())
        pix_dev = pixels.to(device, non_blocking=True)
        meta = [torch.from_numpy(a).pin_memory() for a in (offsets_np, sizes_np, plan_i, plan_f)]
        out = torch.empty((B, 3, S, S), dtype=self.out_dtype, device=device)
        with torch.cuda.device(device):
            rc = _C.lib().cx_image_transform(
                pix_dev.data_ptr(), *(m.data_ptr() for m in meta), out.data_ptr(), int(self.out_dtype == torch.bfloat16), B, S,
                self.mean.ctypes.data_as(_C.C.POINTER(_C.f32)), self.std.ctypes.data_as(_C.C.POINTER(_C.f32)), _C.cur_stream())
            _C.check(rc, "cx_image_transform")
            ev = torch.cuda.Event()
            ev.record()
        self._inflight = [(e, m) for e, m in self._inflight if not e.query()]
        self._inflight.append((ev, meta))
        return out
