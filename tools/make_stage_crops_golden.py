"""Writes tests/golden/stage_crops.pt: small inputs and what the reference's test-time chain makes of them.

    python tools/make_stage_crops_golden.py

The chain is eval/main_classifier.py:456-469 without its random ColorJitter: RandomHorizontalFlip(command) ->
FiveCrop -> Scale(BICUBIC) -> ToTensor, then T.Normalize on the device.  utils/augmentation.py cannot be imported
where this project is developed (torchvision and joblib are absent), so this script makes the PIL calls those
classes make: Image.transpose(FLIP_LEFT_RIGHT), Image.crop, Image.resize(size, Image.BICUBIC); then /255 and
(x - mean) / std in torch fp32 (ToTensor, Normalize).  PIL is needed here only: no test imports it to read the
fixture.

The fixture holds, per case, the frames, the clips' frame indices, the crop boxes and flips, and PIL's resized
BYTES per crop and frame; plus one table `levels` (3, 256) = the torch fp32 value of every byte per channel.  The
expected fp32 tensor is levels[c][byte] (tests/crops_harness.py: golden_expected) -- the float step is a function
of the byte alone, and the table keeps the file at 100 KB instead of 400."""
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coclr_amd.staging import IMAGENET_MEAN, IMAGENET_STD, five_crop_boxes      # noqa: E402


def pil_chain(frame, x0, y0, flip, cw, ch, S):
    img = Image.fromarray(frame)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = img.crop((x0, y0, x0 + cw, y0 + ch))
    return np.asarray(img.resize((S, S), Image.BICUBIC))


def case(frames, frame_index, boxes, flips, cw, ch, S):
    resized = np.stack([np.stack([pil_chain(f, x0, y0, fl, cw, ch, S) for f in frames])
                        for (x0, y0), fl in zip(boxes, flips)])
    return {"frames": torch.from_numpy(frames), "frame_index": torch.tensor(frame_index, dtype=torch.int64),
            "boxes": torch.tensor(boxes, dtype=torch.int32), "flips": torch.tensor(flips, dtype=torch.int32),
            "crop": (cw, ch), "S": S, "resized": torch.from_numpy(resized)}


def main():
    rng = np.random.RandomState(0)
    # A: six 40 x 52 frames (H x W), the last a 0/255 checkerboard of 5 x 7 cells; T = 4, three clips (overlap, left padding);
    # ten crops 28 -> 16 (the production ratio 1.75)
    frames = rng.randint(0, 256, size=(6, 40, 52, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:40, 0:52]
    frames[5] = (((yy // 7 + xx // 5) & 1) * 255).astype(np.uint8)[:, :, None]      # hard edges: overshoot
    boxes = five_crop_boxes(52, 40, 28)
    a = case(frames, [[0, 1, 2, 3], [2, 3, 4, 5], [0, 0, 0, 1]], boxes * 2, [0] * 5 + [1] * 5, 28, 28, 16)
    # B: one 30 x 33 frame (H x W), T = 1: a 12 x 20 box (upscaled in x, 5 taps; downscaled in y) and an identity
    # 16 -> 16 box, each plain and flipped
    frame = rng.randint(0, 256, size=(1, 30, 33, 3)).astype(np.uint8)
    b1 = case(frame, [[0]], [(7, 5), (7, 5)], [0, 1], 12, 20, 16)
    b2 = case(frame, [[0]], [(3, 9), (3, 9)], [0, 1], 16, 16, 16)
    levels = torch.arange(256, dtype=torch.float32)[None, :].expand(3, 256) / 255
    levels = (levels - torch.tensor(IMAGENET_MEAN)[:, None]) / torch.tensor(IMAGENET_STD)[:, None]
    out = os.path.join(ROOT, "tests", "golden", "stage_crops.pt")
    torch.save({"A": a, "B_rect": b1, "B_identity": b2, "levels": levels.contiguous(),
                "pil": PIL.__version__}, out)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
