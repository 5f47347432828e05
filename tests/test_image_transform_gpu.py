"""cx_image_transform (csrc/image.hip) against the float64 yardstick of tests/img_ref.py, and the data path wired into
ImageTextTrainer.

Condition per image, with levels recovered from the fp32 output as round((out * std + mean) * 255):
  * they equal the yardstick's except on at most 0.5 % of the image's values, and none differs by more than 1 level (the kernel's
    weights are fp32: a sum within ~1e-5 of a rounding tie may fall on the other side; the yardstick against PIL stays under
    0.04 % on the shared inputs, tests/test_image_transform_cpu.py);
  * where the levels agree, the fp32 output is within 4 fp32 ulps of the float64 value of (level / 255 - mean) / std (a chain of
    three operations plus headroom), and the bf16 output of a second launch is the bf16 rounding of that value or its neighbour.
An S x S source under the identity plan must come back with exactly its own levels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import img_ref as R

pytestmark = pytest.mark.gpu
ERR_SHAPE = -1
MEAN, STD = np.asarray(R.OPENAI_MEAN, np.float32), np.asarray(R.OPENAI_STD, np.float32)


def _launch(images, plans, S, dtype=torch.float32, pad=None, out=None):
    """One launch over a ragged batch; pad[b] bytes are put in front of image b.  Returns (rc, out on the device)."""
    from contrastors_amd import _C

    pad = pad or [0] * len(images)
    parts, offsets, pos = [], [], 0
    for img, p in zip(images, pad):
        parts += [np.full(p, 0xA5, np.uint8), img.reshape(-1)]
        offsets.append(pos + p)
        pos += p + img.size
    offsets.append(pos)
    pix = torch.from_numpy(np.concatenate(parts)).cuda()
    meta = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (
        np.asarray(offsets, np.int64), np.asarray([im.shape[:2] for im in images], np.int32),
        np.asarray([p[0] for p in plans], np.int32), np.asarray([p[1] for p in plans], np.float64))]
    if out is None:
        out = torch.empty((len(images), 3, S, S), dtype=dtype, device="cuda")
    rc = _C.lib().cx_image_transform(pix.data_ptr(), *(m.data_ptr() for m in meta), out.data_ptr(), int(out.dtype == torch.bfloat16),
                                     len(images), S, MEAN.ctypes.data_as(C.POINTER(C.c_float)),
                                     STD.ctypes.data_as(C.POINTER(C.c_float)), _C.cur_stream())
    torch.cuda.synchronize()   # (the pinned plans live until here)
    return rc, out


def _ordered_bf16(t):
    """bf16 bit patterns as integers that step by one between neighbouring values."""
    bits = t.view(torch.int16).to(torch.int32)
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))


def _judge(name, out32, out16, want_levels):
    """The module docstring's condition for one image: out32 / out16 (3, S, S) fp32 / bf16 on the host, want_levels (S, S, 3)."""
    got = R.levels_of(out32.numpy(), MEAN, STD)
    d = np.abs(got - want_levels)
    print(f"{name}: {int((d > 0).sum())} of {d.size} levels differ, max {d.max():.0f}")
    assert d.max() <= 1, (name, d.max())
    assert (d > 0).mean() <= 0.005, (name, int((d > 0).sum()), d.size)
    agree = torch.from_numpy((got == want_levels).transpose(2, 0, 1).copy())
    exact = torch.from_numpy(R.normalize(want_levels, MEAN, STD))
    ulp = torch.from_numpy(np.spacing(np.abs(exact.numpy()).astype(np.float32)).astype(np.float64))
    err = ((out32.double() - exact).abs() / ulp)[agree]
    assert err.numel() and err.max() <= 4.0, (name, float(err.max()))
    # bf16 cannot be asked for its levels: above 2.0 its spacing (2^-6) is wider than a level's (1 / (255 * 0.276) = 0.0142), so the
    # top blue levels share values.  It is the same computation with one more rounding: where the fp32 launch has the level right,
    # the bf16 launch must hold the bf16 rounding of the exact value, or its neighbour.
    step = (_ordered_bf16(out16) - _ordered_bf16(exact.to(torch.float32).to(torch.bfloat16))).abs()[agree]
    assert step.max() <= 1, (name, int(step.max()))


def _cases(S):
    """[(name, image, plan)]: every source under its eval plan and as a whole-image crop, crops on each border, the identity;
    ordered so that the 1 x 1 image sits between large ones."""
    from contrastors_amd.image_transform import eval_plan, train_plan

    def src(h, w, seed):
        return R.noise_image(h, w, seed)

    big, wide, tall = src(300, 517, 1), src(37, 500, 2), src(61, 83, 3)
    cases = [("300x517-16x", big, train_plan((3, 5, min(297, 16 * S - 1), min(511, 16 * S - 1)), S)),   # (scale just under 16 at S = 16)
             ("300x517-eval", big, eval_plan(300, 517, S)),                       # (fractional origin: 517 -> int(S * 517 / 300))
             ("1x1-eval", src(1, 1, 4), eval_plan(1, 1, S)),
             ("37x500-eval", wide, eval_plan(37, 500, S)),
             ("300x517-crop", big, train_plan((0, 0, 300, 517), S)),
             ("1x1-crop", src(1, 1, 5), train_plan((0, 0, 1, 1), S)),
             ("37x500-crop", wide, train_plan((0, 0, 37, 500), S)),
             ("5x7-up", src(5, 7, 6), train_plan((0, 0, 5, 7), S)),
             ("9x13-eval", src(9, 13, 7), eval_plan(9, 13, S)),
             ("9x13-crop", src(9, 13, 7), train_plan((2, 3, 5, 7), S)),
             ("61x83-eval", tall, eval_plan(61, 83, S)),                            # (83 -> 43 at S = 32: origin 6 * 83 / 43)
             ("61x83-top", tall, train_plan((0, 10, 31, 41), S)),
             ("61x83-bottom", tall, train_plan((30, 10, 31, 41), S)),
             ("61x83-left", tall, train_plan((10, 0, 31, 41), S)),
             ("61x83-right", tall, train_plan((10, 42, 31, 41), S)),
             ("300x517-inner", big, train_plan((61, 74, 187, 339), S)),
             ("pattern-eval", R.pattern_image(), eval_plan(47, 61, S)),
             ("identity", src(S, S, 8), ((0, S, 0, S), (0.0, 1.0, 0.0, 1.0)))]
    # the kernel serves a scale up to 16 per axis: at S = 16 and 32 the whole 300 x 517 and 37 x 500 images are beyond it (their
    # crops above are not); test_out_of_range_is_refused_and_served_on_the_host covers that side
    return [c for c in cases if max(c[2][1][1], c[2][1][3]) <= 16.0]


@pytest.fixture(scope="module")
def yardstick():
    cache = {}

    def get(name, img, plan, S):
        key = (name, S)
        if key not in cache:
            cache[key] = R.resize_levels(img, plan[0], plan[1], S)
        return cache[key]
    return get


@pytest.mark.parametrize("S", [16, 32, 224])
def test_kernel_matches_the_yardstick(S, yardstick):
    cases = _cases(S)
    images, plans = [c[1] for c in cases], [c[2] for c in cases]
    # byte offsets of every residue mod 4: the images' own sizes (3 h w) already vary; the pads make sure of 0, 1, 2, 3 up front
    pad = [(b % 4) for b in range(len(cases))]
    starts = np.cumsum([p + (images[b - 1].size if b else 0) for b, p in enumerate(pad)])
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    rc32, out32 = _launch(images, plans, S, torch.float32, pad)
    rc16, out16 = _launch(images, plans, S, torch.bfloat16, pad)
    assert rc32 == 0 and rc16 == 0
    out32, out16 = out32.cpu(), out16.cpu()
    for b, (name, img, plan) in enumerate(cases):
        want = yardstick(name, img, plan, S)
        if name == "identity":
            assert np.array_equal(want, img.astype(np.float64))
            assert np.array_equal(R.levels_of(out32[b].numpy(), MEAN, STD), want)
        _judge(f"S={S} {name}", out32[b], out16[b], want)
    # a group launched on its own gives what it gave inside the mixed batch, whatever its offset and neighbours were
    solo = [0, 1, 6]
    rc, out = _launch([images[i] for i in solo], [plans[i] for i in solo], S, torch.float32)
    assert rc == 0 and torch.equal(out.cpu(), out32[solo])


def test_large_source_single_image(yardstick):
    from contrastors_amd.image_transform import eval_plan

    img, S = R.noise_image(1024, 1365, 11), 224
    plan = eval_plan(1024, 1365, S)
    rc32, out32 = _launch([img], [plan], S, torch.float32)
    rc16, out16 = _launch([img], [plan], S, torch.bfloat16)
    assert rc32 == 0 and rc16 == 0
    _judge("1024x1365 -> 224", out32[0].cpu(), out16[0].cpu(), yardstick("1024x1365", img, plan, S))


def test_two_launches_give_the_same_bits():
    cases = _cases(32)
    images, plans = [c[1] for c in cases], [c[2] for c in cases]
    for dtype in (torch.float32, torch.bfloat16):
        (_, a), (_, b) = _launch(images, plans, 32, dtype), _launch(images, plans, 32, dtype)
        assert torch.equal(a, b)


def test_out_of_range_is_refused_and_served_on_the_host(yardstick):
    from contrastors_amd.image_transform import GpuImageTransform, eval_plan, train_plan

    strip, S = R.noise_image(16, 2048, 12), 16
    plan = train_plan((0, 0, 16, 2048), S)                      # x scale 128
    sentinel = torch.full((1, 3, S, S), 7.0, device="cuda")
    rc, out = _launch([strip], [plan], S, out=sentinel.clone())
    assert rc == ERR_SHAPE and torch.equal(out, sentinel)
    ok = R.noise_image(40, 40, 13)
    big = torch.full((1, 3, 1024, 1024), 7.0, device="cuda")
    rc, out = _launch([ok], [eval_plan(40, 40, 1024)], 1024, out=big.clone())
    assert rc == ERR_SHAPE and torch.equal(out, big)
    # the same strip through GpuImageTransform: resized on the host to the same plan, counted; its neighbour goes through the kernel
    t = GpuImageTransform(S, is_train=False, out_dtype=torch.float32)
    plans = [plan, eval_plan(40, 40, S)]
    vision = {"pixels_u8": torch.from_numpy(np.concatenate([strip.reshape(-1), ok.reshape(-1)])),
              "offsets": torch.tensor([0, strip.size, strip.size + ok.size]), "sizes": torch.tensor([[16, 2048], [40, 40]], dtype=torch.int32)}
    out = t(vision, plans=([p[0] for p in plans], [p[1] for p in plans])).cpu()
    assert t.host_fallbacks == 1 and out.shape == (2, 3, S, S)
    for b, (name, img) in enumerate((("strip", strip), ("40x40", ok))):
        d = np.abs(R.levels_of(out[b].numpy(), MEAN, STD) - yardstick(name, img, plans[b], S))
        print(f"{name}: {int((d > 0).sum())} of {d.size} levels differ, max {d.max():.0f}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.005


VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(20)]


def test_trainer_step_from_tar_shards(tmp_path):
    """tar shard -> loader -> ragged batch -> ImageTextTrainer.training_step (transform on the GPU, tiny towers): the loss is
    finite and bit-identical to the same step of an identically built trainer fed the dense tensor GpuImageTransform gives for
    that batch; a second batch runs too."""
    from transformers import BertTokenizer

    from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs, TransformsConfig
    from contrastors_amd.image_data import TarImageTextDataset
    from contrastors_amd.image_transform import GpuImageTransform
    from contrastors_amd.nomic_bert import NomicBertConfig
    from contrastors_amd.trainers import ImageTextTrainer
    from contrastors_amd.vit import ViTConfig
    from oracle.make_golden import TINY_NOMIC

    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(str(tmp_path / "vocab.txt"), do_lower_case=True)
    members = []
    for k in range(16):
        members += [(f"{k:04d}.png", R.png_bytes(R.noise_image(33 + 3 * k, 70 - 2 * k, 900 + k))),
                    (f"{k:04d}.txt", f"w{k} w{(3 * k) % 20} w{(7 * k) % 20}".encode())]
    R.write_tar(tmp_path / "000.tar", members)
    cfg = Config(train_args=TrainArgs(learning_rate=2e-3, weight_decay=0.01, warmup_steps=0, grad_cache=False,
                                      schedule_type="linear", max_grad_norm=1.0, clamp_logits=True),
                 data_args=DataArgs(batch_size=8, seed=7, image_text_shards=str(tmp_path / "000.tar")),
                 text_model_args=ModelArgs(logit_scale=20.0, pooling="mean", model_name="tiny-text", seq_len=24),
                 vision_model_args=ModelArgs(logit_scale=20.0, pooling="cls", model_name="tiny-vit", trainable_logit_scale=True),
                 transforms=TransformsConfig(image_size=32, aug_cfg={"scale": (0.5, 1.0)}))
    tc = NomicBertConfig(**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__})
    vc = ViTConfig(n_embd=256, n_layer=1, n_head=4, n_inner=512, img_size=32, patch_size=8)
    ds = TarImageTextDataset(cfg.data_args.image_text_shards, 8, tokenizer=tok, seq_len=24, seed=7)
    first, second = list(ds)
    assert first["vision"]["pixels_u8"].dtype == torch.uint8 and first["text"]["input_ids"].shape == (8, 24)
    a = ImageTextTrainer(cfg, torch.bfloat16, device="cuda", text_trunk_config=tc, vision_trunk_config=vc, total_steps=20)
    assert a.image_transform.image_size == 32 and a.image_transform.scale == (0.5, 1.0)
    loss_a = a.training_step(first)
    dense = GpuImageTransform.from_config(cfg.transforms, is_train=True, seed=7)(first["vision"])   # the trainer's seed on rank 0
    assert dense.shape == (8, 3, 32, 32) and dense.dtype == torch.bfloat16
    b = ImageTextTrainer(cfg, torch.bfloat16, device="cuda", text_trunk_config=tc, vision_trunk_config=vc, total_steps=20)
    loss_b = b.training_step({"text": first["text"], "vision": {"input_ids": dense}})
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    assert torch.isfinite(a.training_step(second))
    assert a.image_transform.host_fallbacks == 0
