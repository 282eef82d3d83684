"""Write tests/golden/resize_pad_small.npz: three small uint8 videos of different sizes and what the REFERENCE's own input transform
makes of them -- ImageResize(48, "bilinear") then ImagePad(48, 48), src/datasets/data_utils.py:112-253, executed from the reference's
source (oracle/ref_functions.py; needs the reference tree) on the float frames exactly as _load_video does
(src/datasets/dataset_base.py:270-273).  The fixture is data only: inputs and the recorded fp32 output.  It is the link between the
reference and the GPU run of tests/test_resize_pack.py::test_recorded_reference_fixture, where the reference tree does not exist.

    python tools/make_resize_golden.py            # rewrites the fixture (deterministic)
"""
import numbers
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.modules.utils import _quadruple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "resize_pad_small.npz")
S = 48
VIDEOS = [(2, 40, 64), (1, 72, 48), (2, 56, 56)]            # (T, h, w): landscape, portrait, square (every one is resampled)


def reference_transform(max_img_size):
    from oracle import ref_functions as RF
    ns = RF.load(RF.DATA_UTILS, ["get_padding", "ImagePad", "get_resize_size", "ImageResize"],
                 extra_ns=dict(Image=SimpleNamespace(BILINEAR=2), img_tensor_resize=F.interpolate, img_tensor_pad=F.pad, _quadruple=_quadruple,
                               numbers=numbers, img_resize=None, img_pad=None))
    resize, pad = ns["ImageResize"](max_img_size, "bilinear"), ns["ImagePad"](max_img_size, max_img_size)
    return lambda frames_u8: pad(resize(frames_u8.float()))


def main():
    tf = reference_transform(S)
    arrays = dict(max_img_size=np.int64(S))
    for i, (t, h, w) in enumerate(VIDEOS):
        g = torch.Generator().manual_seed(100 + i)
        v = torch.randint(0, 256, (t, 3, h, w), generator=g, dtype=torch.uint8)
        arrays[f"video{i}"] = v.numpy()
        arrays[f"padded{i}"] = tf(v).numpy()
        assert arrays[f"padded{i}"].shape == (t, 3, S, S) and arrays[f"padded{i}"].dtype == np.float32
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
