"""Microbenchmark of the image data path's split: the GPU crop-resize-normalize kernel against what it replaces
on the host, and the decode that stays there.

    python scripts/image_transform_microbench.py [--batch 2048] [--height 384] [--width 512] [--size 224] [--reps 31] [--out FILE]

  (1) cx_image_transform: B seeded noise sources -> (B, 3, S, S) bf16 under seeded RandomResizedCrop plans (scale 0.9-1), device
      events around each launch, median of `reps` (>= 7) after 3 warm-up launches; images / s.
  (2) the kernel's bytes moved (the crops' pixels read once + the output written) over that time, as a fraction of the HBM copy
      rate of the same box measured the way scripts/box_calibration.py does (cx_calib_copy, 1 GiB read + 1 GiB written, median of 10).
  (3) host: the reference chain per image with PIL + torch on ONE core (crop, resize BICUBIC, float / 255, normalize, CHW), x 16.
  (4) host: decode only (Image.open(jpeg).convert("RGB") -> uint8 array) per core, for the same images as JPEG (quality 90) and for
      a low-pass version of them (noise is the worst case for a JPEG decoder; photographs sit nearer the smooth figure).
Needs the GPU: there is no fallback.  One JSON line at the end."""
from __future__ import annotations

import argparse
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from contrastors_amd import _C  # noqa: E402
from contrastors_amd.image_transform import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, GpuImageTransform  # noqa: E402


def hbm_copy_rate(nbytes=1 << 30):
    lib, s = _C.lib(), _C.cur_stream()
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    for _ in range(3):
        _C.check(lib.cx_calib_copy(src.data_ptr(), dst.data_ptr(), nbytes, s), "cx_calib_copy")
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
    ev[0].record()
    for i in range(10):
        _C.check(lib.cx_calib_copy(src.data_ptr(), dst.data_ptr(), nbytes, s), "cx_calib_copy")
        ev[i + 1].record()
    torch.cuda.synchronize()
    return 2.0 * nbytes / (statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(10)) * 1e-3)


def per_image_seconds(fn, items, min_seconds=2.0):
    """Wall time per item of fn over `items`, repeated until at least min_seconds have been timed (after one untimed pass)."""
    for it in items[:4]:
        fn(it)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_seconds:
        for it in items:
            fn(it)
        n += len(items)
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--host-images", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_transform_microbench needs the GPU")
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    from PIL import Image

    B, H, W, S = args.batch, args.height, args.width, args.size
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    pixels = torch.from_numpy(rng.integers(0, 256, B * H * W * 3, dtype=np.uint8))
    vision = {"pixels_u8": pixels.cuda(), "offsets": torch.arange(B + 1, dtype=torch.int64) * (3 * H * W),
              "sizes": torch.tensor([[H, W]] * B, dtype=torch.int32)}
    t = GpuImageTransform(S, is_train=True, out_dtype=torch.bfloat16, seed=0)
    plan_i, plan_f = t.plans(vision["sizes"])
    out = t(vision, plans=(plan_i, plan_f))      # (through the public call once: the plans are served, nothing falls back)
    lib, stream = _C.lib(), _C.cur_stream()
    meta = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (vision["offsets"].numpy(), vision["sizes"].numpy(), plan_i, plan_f)]
    mean3, std3 = (np.asarray(v, np.float32) for v in (OPENAI_DATASET_MEAN, OPENAI_DATASET_STD))
    fp = _C.C.POINTER(_C.f32)

    def launch():
        _C.check(lib.cx_image_transform(vision["pixels_u8"].data_ptr(), *(m.data_ptr() for m in meta), out.data_ptr(), 1, B, S,
                                        mean3.ctypes.data_as(fp), std3.ctypes.data_as(fp), stream), "cx_image_transform")

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    kernel_ms = statistics.median(ms)
    crop_bytes = int(3 * ((plan_i[:, 1] - plan_i[:, 0]).astype(np.int64) * (plan_i[:, 3] - plan_i[:, 2])).sum())
    moved = crop_bytes + out.numel() * out.element_size()
    copy_rate = hbm_copy_rate()

    # host side, one core: the first images of the same batch under the same plans
    n = min(args.host_images, B)
    imgs = [pixels[b * 3 * H * W:(b + 1) * 3 * H * W].numpy().reshape(H, W, 3) for b in range(n)]
    mean = torch.tensor(OPENAI_DATASET_MEAN).view(3, 1, 1)
    std = torch.tensor(OPENAI_DATASET_STD).view(3, 1, 1)

    def chain(b):
        y0, y1, x0, x1 = (int(v) for v in plan_i[b])
        im = Image.fromarray(imgs[b]).crop((x0, y0, x1, y1)).resize((S, S), Image.BICUBIC).convert("RGB")
        x = torch.from_numpy(np.asarray(im)).permute(2, 0, 1).float().div_(255.0)   # ToTensor
        return x.sub_(mean).div_(std)                                                 # Normalize

    chain_s = per_image_seconds(chain, list(range(n)))

    def jpeg(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90)
        return buf.getvalue()

    def smooth(img):   # 8 x 8 block means, upsampled: photograph-like low-frequency content
        small = Image.fromarray(img).resize((W // 8, H // 8), Image.BOX)
        return np.asarray(small.resize((W, H), Image.BICUBIC))

    def decode(data):
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    noise_jpegs, smooth_jpegs = [jpeg(i) for i in imgs], [jpeg(smooth(i)) for i in imgs]
    dec_noise_s, dec_smooth_s = per_image_seconds(decode, noise_jpegs), per_image_seconds(decode, smooth_jpegs)

    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "source": [H, W], "size": S, "reps": args.reps,
           "kernel_ms_median": kernel_ms, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
           "kernel_images_per_s": B / (kernel_ms * 1e-3), "kernel_bytes_moved": moved,
           "kernel_tb_per_s": moved / (kernel_ms * 1e-3) / 1e12, "hbm_copy_tb_per_s": copy_rate / 1e12,
           "kernel_fraction_of_copy_rate": moved / (kernel_ms * 1e-3) / copy_rate,
           "host_chain_images_per_s_per_core": 1.0 / chain_s, "host_chain_images_per_s_x16": 16.0 / chain_s,
           "host_decode_noise_images_per_s_per_core": 1.0 / dec_noise_s, "host_decode_noise_images_per_s_x16": 16.0 / dec_noise_s,
           "host_decode_smooth_images_per_s_per_core": 1.0 / dec_smooth_s, "host_decode_smooth_images_per_s_x16": 16.0 / dec_smooth_s,
           "jpeg_kb_noise": sum(map(len, noise_jpegs)) / n / 1e3, "jpeg_kb_smooth": sum(map(len, smooth_jpegs)) / n / 1e3,
           "host_fallbacks": t.host_fallbacks}
    line = json.dumps(rec)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
