#!/usr/bin/env python3
"""Generate tests/golden/px_*.npz by RUNNING the reference's still pixmap sources.

Run in the build container only (the reference package does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_px.py

transflow/pixmap/still.py imports cv2 at its top (VideoStillPixmapSource alone uses it) and source.py annotates with
typing.Self: an empty stub module named cv2 goes into sys.modules and, on Python 3.10, typing.Self = typing.Any is set
BEFORE the reference is imported.  Every pixel of every fixture is made by the reference's own classes, entered and
asked for one frame.  A fixture holds the class, the seed, the size, the colour string, the gradient's tree as numbers
(postfix rows of type, a, b, c), the image a source or an alteration was read from, and the array that came out: data
only.  Every fixture stays under 64 x 96 pixels.
"""
import os
import random
import shutil
import sys
import tempfile
import types
import typing

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import px_ref  # noqa: E402


def reference_classes():
    if not hasattr(typing, "Self"):
        typing.Self = typing.Any
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from transflow.pixmap import still
    return still


def overlay_image(height, width, seed):
    """RGBA overlay: random colours, about half of the pixels with alpha 0, the others with alpha 1..255."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
    img[:, :, 3] = np.where(rng.random((height, width)) < 0.5, 0, rng.integers(1, 256, (height, width)))
    return img


def save_png(array, directory, name):
    import PIL.Image
    path = os.path.join(directory, name)
    PIL.Image.fromarray(array).save(path)
    return path


def main():
    still = reference_classes()
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="px-golden-")
    saved_np, saved_py = np.random.get_state(), random.getstate()

    def run(source):
        with source as s:
            array = next(s)
        assert array.dtype == np.uint8 and array.ndim == 3
        return array

    def write(name, **arrays):
        path = os.path.join(OUT, f"px_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {arrays['array'].shape}, {os.path.getsize(path)} B")

    def meta(kind, height, width, seed=-1, color=""):
        return dict(kind=np.str_(kind), height=np.int64(height), width=np.int64(width), seed=np.int64(seed),
                    color=np.str_(color))

    for seed, h, w in px_ref.GRADIENT_CASES:
        src = still.GradientPixmapSource(w, h, seed)
        array = run(src)
        random.seed(seed)
        tree = src.generate(src.NODE_TRIPLE, 5)          # the tree _init_array drew, drawn again by the same method
        write(f"gradient_s{seed}_{h}x{w}", array=array, tree=px_ref.tree_rows(tree), **meta("gradient", h, w, seed))

    h, w = 37, 53
    for seed in (0, 3):
        for kind, cls in (("noise", still.NoisePixmapSource), ("bwnoise", still.BwNoisePixmapSource),
                          ("cnoise", still.ColoredNoisePixmapSource)):
            write(f"{kind}_s{seed}", array=run(cls(w, h, seed)), **meta(kind, h, w, seed))
        write(f"color_random_s{seed}", array=run(still.ColorPixmapSource(w, h, None, seed)), **meta("color", h, w, seed))
    for name, string in (("hex", "#102030"), ("rgb", "rgb(200, 17, 3)"), ("tuple", "(1,2,255)"), ("barehex", "a0b1c2")):
        write(f"color_{name}", array=run(still.ColorPixmapSource(w, h, string, seed=5)), **meta("color", h, w, 5, string))

    for name, channels in (("rgb", 3), ("rgba", 4)):
        image = np.random.default_rng(40 + channels).integers(0, 256, (20, 30, channels), dtype=np.uint8)
        array = run(still.ImagePixmapSource(save_png(image, tmp, f"image_{name}.png")))
        write(f"image_{name}", array=array, image=image, **meta("image", 20, 30))

    for name, (oh, ow) in (("same", (37, 53)), ("smaller", (11, 19))):
        overlay = overlay_image(oh, ow, 50 + oh)
        array = run(still.ColoredNoisePixmapSource(w, h, 9, save_png(overlay, tmp, f"overlay_{name}.png")))
        write(f"altered_{name}", array=array, overlay=overlay, **meta("cnoise", h, w, 9))
    # an overlay over a 4-channel pixmap: the reference's index stays (i * width + j) * 3 (source.py:57)
    image = np.random.default_rng(61).integers(0, 256, (20, 30, 4), dtype=np.uint8)
    overlay = overlay_image(7, 9, 62)
    array = run(still.ImagePixmapSource(save_png(image, tmp, "image_altered.png"), save_png(overlay, tmp, "overlay_rgba.png")))
    write("image_rgba_altered", array=array, image=image, overlay=overlay, **meta("image", 20, 30))

    np.random.set_state(saved_np)
    random.setstate(saved_py)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
