"""Writes tests/golden/jpeg_ragged.pt: the RAW bytes of four seeded synthetic frames at the sizes kinetics400-256 holds
(a 256-pixel short side and the video's own aspect ratio: dataset/convert_video_to_lmdb.py:110-115 of the reference)
-- 340 x 256, 454 x 256, 256 x 340 and 320 x 256 (W x H), 4:2:0, quality 75 -- as PIL (libjpeg-turbo) encodes them.

    python tools/make_ragged_golden.py

Bytes only: the expected frames are what the one-size jpeg.decode makes of them, which tests/golden/jpeg_frames.pt
already pins to PIL's decoder.  tools/ragged_step.py builds its mixed batch from these and the 320 x 240 frame of
jpeg_frames.pt; tests/test_gpu_ragged.py decodes the four in one ragged call.  PIL is needed here only."""
import os

import PIL
import torch
from PIL import features

import make_jpeg_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_ragged.pt")
SIZES = ((340, 256), (454, 256), (256, 340), (320, 256))            # W x H


def main():
    assert features.check_feature("libjpeg_turbo")
    cases = []
    for k, (W, H) in enumerate(SIZES):
        raw = G.encode(G.content("mild", W, H, 4001 + k), "4:2:0", quality=75)
        cases.append({"name": "%dx%d_420_q75" % (W, H), "raw": torch.frombuffer(bytearray(raw), dtype=torch.uint8),
                      "width": W, "height": H, "ncomp": 3, "sampling": (2, 2)})
    torch.save({"pil": PIL.__version__, "libjpeg_turbo": features.version_feature("libjpeg_turbo"), "cases": cases}, OUT)
    print("wrote %s (%d bytes, %d cases)" % (OUT, os.path.getsize(OUT), len(cases)))
    assert os.path.getsize(OUT) <= 100000


if __name__ == "__main__":
    main()
