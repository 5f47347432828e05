"""NumPy float64 yardstick of the image transform: PIL's two-pass BICUBIC resize with its 8-bit intermediate,
then normalize.  Shared by tests/test_image_transform_cpu.py (yardstick against PIL) and tests/test_image_transform_gpu.py
(kernel against yardstick).  The keyword switches plant one error each; a test shows that its condition catches them.

A plan is (plan_i, plan_f) = ((y_lo, y_hi, x_lo, x_hi), (y_origin, y_scale, x_origin, x_scale)), as the kernel takes it.
"""
from __future__ import annotations

import numpy as np

OPENAI_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_STD = (0.26862954, 0.26130258, 0.27577711)


def _cubic(t: np.ndarray) -> np.ndarray:
    a = -0.5
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0,
                    np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


def axis_taps(lo: int, hi: int, origin: float, scale: float, S: int, *, no_half=False, fixed_support=False,
              unnormalised=False):
    """Per output pixel: (first source index, float64 weights)."""
    fs = max(float(scale), 1.0)
    support = 2.0 if fixed_support else 2.0 * fs
    out = []
    for o in range(S):
        c = float(origin) + (o + (0.0 if no_half else 0.5)) * float(scale)
        xmin = max(int(c - support + 0.5), lo)
        xmax = min(int(c + support + 0.5), hi)
        x = np.arange(xmin, xmax, dtype=np.float64)
        w = _cubic((x - c + 0.5) / fs)
        if not unnormalised and w.size and w.sum() != 0.0:
            w = w / w.sum()
        out.append((xmin, w))
    return out


def _round_levels(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(v + 0.5), 0.0, 255.0)


def resize_levels(img: np.ndarray, plan_i, plan_f, S: int, *, no_intermediate_rounding=False, whole_image_clamp=False,
                  **planted) -> np.ndarray:
    """img: (H, W, 3) uint8 -> (S, S, 3) float64 levels 0..255 (integers)."""
    H, W, _ = img.shape
    y_lo, y_hi, x_lo, x_hi = (int(v) for v in plan_i)
    y_origin, y_scale, x_origin, x_scale = (float(v) for v in plan_f)
    if whole_image_clamp:
        y_lo, y_hi, x_lo, x_hi = 0, H, 0, W
    src = img.astype(np.float64)
    xt = axis_taps(x_lo, x_hi, x_origin, x_scale, S, **planted)
    yt = axis_taps(y_lo, y_hi, y_origin, y_scale, S, **planted)
    r0, r1 = min(t[0] for t in yt), max(t[0] + t[1].size for t in yt)
    inter = np.zeros((H, S, 3))
    for o, (x0, w) in enumerate(xt):
        inter[r0:r1, o] = np.tensordot(w, src[r0:r1, x0:x0 + w.size], axes=(0, 1)) if w.size else 0.0
    if not no_intermediate_rounding:
        inter = _round_levels(inter)
    out = np.zeros((S, S, 3))
    for o, (y0, w) in enumerate(yt):
        out[o] = np.tensordot(w, inter[y0:y0 + w.size], axes=(0, 0)) if w.size else 0.0
    return _round_levels(out)


def normalize(levels: np.ndarray, mean=OPENAI_MEAN, std=OPENAI_STD) -> np.ndarray:
    """(S, S, 3) levels -> (3, S, S) float64, with mean / std taken at their fp32 values (what the kernel is given)."""
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    return np.ascontiguousarray(((levels / 255.0 - m) / s).transpose(2, 0, 1))


def levels_of(out: np.ndarray, mean=OPENAI_MEAN, std=OPENAI_STD) -> np.ndarray:
    """(3, S, S) normalised values -> (S, S, 3) integer levels, round((out * std + mean) * 255)."""
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    return np.rint((np.asarray(out, np.float64).transpose(1, 2, 0) * s + m) * 255.0)


def png_bytes(img: np.ndarray) -> bytes:
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")   # lossless: the loader hands back exactly these pixels
    return buf.getvalue()


def write_tar(path, members) -> None:
    """members: [(name, bytes)] in order -> an uncompressed tar shard."""
    import io
    import tarfile

    with tarfile.open(path, "w") as tf:
        for name, data in members:
            info = tarfile.TarInfo(name)
            info.size = len(data)
            tf.addfile(info, io.BytesIO(data))


def noise_image(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pattern_image(h: int = 47, w: int = 61) -> np.ndarray:
    """Checkerboard (sharp edges: over- and undershoot of the cubic, so both clamps act) in red, gradients in green / blue.
    Prime sides: at 48 x 64 the scales to 16 and 32 are 3 and 3 / 2, the weights small rationals, and the regular data puts
    dozens of values exactly on a rounding tie -- which PIL decides by its fixed-point weights (see test_image_transform_cpu)."""
    y, x = np.mgrid[0:h, 0:w]
    r = (((y // 4) + (x // 4)) % 2) * 255
    g = (x * 255) // max(w - 1, 1)
    b = (y * 255) // max(h - 1, 1)
    return np.stack([r, g, b], -1).astype(np.uint8)
