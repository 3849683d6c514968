"""Vectorised numpy restatement of the reference's still pixmap sources (transflow/pixmap/still.py) and of the
alteration overlay (transflow/pixmap/source.py:40-69).

The reference fills the gradient with a Python loop over the pixels (still.py:157-162), every value a chain of Python
float operations.  A Python float operation is one IEEE-754 binary64 operation, and so is the numpy operation on a
float64 array: the same chain over whole (H, W) arrays gives the same bits.  `i / (height - 1)` is Python's int / int,
the correctly rounded quotient -- the float64 division of the two (exactly represented) integers.  The byte is numpy's
store of a Python float into a uint8 array: truncation toward zero.  tests/golden/px_*.npz hold what the reference's
own classes returned (tools/capture_golden_px.py); tests/test_px_ref.py compares.

The random draws are numpy's and `random`'s global streams, call for call as the reference makes them."""
import random

import numpy as np

NODE_I, NODE_J, NODE_RGB, NODE_MIX, NODE_TRIPLE, NODE_Z, NODE_B = range(7)      # still.py:86-92
IS_INNER = (NODE_MIX, NODE_TRIPLE)

# seed, height, width of the gradient fixtures
GRADIENT_CASES = [(0, 37, 53), (1, 20, 30), (2, 9, 200), (7, 64, 96), (11, 2, 2), (5, 45, 61)]


# ---- colours and noises (still.py:37-81) ----------------------------------------------------------------------------
def parse_color(string):
    """utils.py:316-324 without the table of names (the fixtures use none)."""
    import re
    m = re.match(r"^(?:rgb)?\((\d+), ?(\d+), ?(\d+)\)$", string, re.IGNORECASE)
    if m is not None:
        return int(m.group(1)), int(m.group(2)), int(m.group(3))
    x = int(string.replace("#", "").replace("0x", "").replace("x", ""), 16)
    return (x >> 16) & 255, (x >> 8) & 255, x & 255


def color(height, width, color_string=None, seed=None):
    np.random.seed(seed)
    rgb = list(np.random.randint(0, 256, size=3, dtype=np.uint8)) if color_string is None else parse_color(color_string)
    array = np.zeros((height, width, 3), dtype=np.uint8)
    array[:, :, :] = rgb
    return array


def noise(height, width, seed=None):
    np.random.seed(seed)
    return np.repeat(np.random.randint(0, 256, size=(height, width, 1), dtype=np.uint8), 3, axis=2)


def bwnoise(height, width, seed=None):
    np.random.seed(seed)
    return np.repeat(np.random.choice([0, 255], size=(height, width, 1)), 3, axis=2).astype(np.uint8)


def cnoise(height, width, seed=None):
    np.random.seed(seed)
    return np.random.randint(0, 256, size=(height, width, 3), dtype=np.uint8)


# ---- the gradient (still.py:84-163) -----------------------------------------------------------------------------------
def generate(node_type=NODE_TRIPLE, depth=5):
    """still.py:94-119; nested tuples (type, a, b, c) as the reference's."""
    if depth <= 0 and node_type != NODE_Z:
        return generate(NODE_Z, 0)
    if node_type in IS_INNER:
        return (node_type, generate(NODE_B, depth - 1), generate(NODE_B, depth - 1), generate(NODE_B, depth - 1))
    if node_type == NODE_B:
        return generate(NODE_Z, depth - 1) if random.random() < .25 else generate(NODE_MIX, depth - 1)
    x = random.random()
    if x < .333:
        return (NODE_I, None, None, None)
    if x < .666:
        return (NODE_J, None, None, None)
    return (NODE_RGB, random.random() * 2 - 1, random.random() * 2 - 1, random.random() * 2 - 1)


def gradient_tree(seed):
    random.seed(seed)
    return generate(NODE_TRIPLE, 5)


def flatten(tree):
    """Postfix rows (type, a, b, c), children before their parent; numbers 0.0 where a node has none."""
    nt, a, b, c = tree
    if nt in IS_INNER:
        return flatten(a) + flatten(b) + flatten(c) + [(nt, 0.0, 0.0, 0.0)]
    return [(nt, a, b, c)] if nt == NODE_RGB else [(nt, 0.0, 0.0, 0.0)]


def unflatten(rows):
    stack = []
    for nt, a, b, c in rows:
        nt = int(nt)
        if nt in IS_INNER:
            kids = stack[-3:]
            assert len(kids) == 3
            del stack[-3:]
            stack.append((nt, *kids))
        else:
            stack.append((nt, float(a), float(b), float(c)) if nt == NODE_RGB else (nt, None, None, None))
    assert len(stack) == 1
    return stack[0]


def tree_rows(tree):
    return np.array(flatten(tree), dtype=np.float64).reshape(-1, 4)


def count_nodes(tree):
    return len(flatten(tree))


def _evaluate(tree, height, width):
    """still.py:121-149 for all pixels at once: three float64 arrays that broadcast to (H, W)."""
    nt, a, b, c = tree
    if nt == NODE_TRIPLE:
        return (_evaluate(a, height, width)[0], _evaluate(b, height, width)[1], _evaluate(c, height, width)[2])
    if nt == NODE_MIX:
        ea, eb, ec = (_evaluate(t, height, width) for t in (a, b, c))
        out = []
        for k in range(3):
            w = (1 + ea[k]) / 2
            out.append((1 - w) * eb[k] + w * ec[k])
        return tuple(out)
    if nt == NODE_RGB:
        return (np.float64(a), np.float64(b), np.float64(c))
    if nt == NODE_I:
        if height - 1 == 0:
            raise ZeroDivisionError("division by zero")
        z = 2 * (np.arange(height, dtype=np.float64)[:, None] / np.float64(height - 1)) - 1
        return (z, z, z)
    if nt == NODE_J:
        if width - 1 == 0:
            raise ZeroDivisionError("division by zero")
        z = 2 * (np.arange(width, dtype=np.float64)[None, :] / np.float64(width - 1)) - 1
        return (z, z, z)
    raise NotImplementedError(f"Unknown node type {nt}")


def gradient_from_tree(tree, height, width):
    array = np.zeros((height, width, 3), dtype=np.uint8)
    if height == 0 or width == 0:
        return array
    for k, v in enumerate(_evaluate(tree, height, width)):
        x = 255 * (v + 1) / 2
        # numpy's store of a float64 into a uint8: truncation toward zero (to a C integer, its low byte)
        array[:, :, k] = np.broadcast_to(np.trunc(x).astype(np.int32).astype(np.uint8), (height, width))
    return array


def gradient(height, width, seed=None):
    return gradient_from_tree(gradient_tree(seed), height, width)


def _evaluate_pixel(tree, i, j, height, width):
    """still.py:121-149 as written: one pixel, Python floats."""
    nt, a, b, c = tree
    if nt == NODE_TRIPLE:
        return (_evaluate_pixel(a, i, j, height, width)[0], _evaluate_pixel(b, i, j, height, width)[1],
                _evaluate_pixel(c, i, j, height, width)[2])
    if nt == NODE_MIX:
        out = [0, 0, 0]
        evals = [_evaluate_pixel(a, i, j, height, width), _evaluate_pixel(b, i, j, height, width),
                 _evaluate_pixel(c, i, j, height, width)]
        for k in range(3):
            w = (1 + evals[0][k]) / 2
            out[k] = (1 - w) * evals[1][k] + w * evals[2][k]
        return (out[0], out[1], out[2])
    if nt == NODE_RGB:
        return (a, b, c)
    if nt == NODE_I:
        z = 2 * (i / (height - 1)) - 1
        return (z, z, z)
    if nt == NODE_J:
        z = 2 * (j / (width - 1)) - 1
        return (z, z, z)
    raise NotImplementedError(f"Unknown node type {nt}")


def gradient_loop(tree, height, width):
    """still.py:156-163 as written, the Python loop over the pixels: what the vectorised form above restates, and what
    tools/bench_pixmap.py times as the reference's per-pixel cost where the reference itself is absent."""
    array = np.zeros((height, width, 3), dtype=np.uint8)
    for i in range(height):
        for j in range(width):
            r, g, b = _evaluate_pixel(tree, i, j, height, width)
            array[i, j, 0] = 255 * (r + 1) / 2
            array[i, j, 1] = 255 * (g + 1) / 2
            array[i, j, 2] = 255 * (b + 1) / 2
    return array.astype(np.uint8)


# ---- the alteration overlay (source.py:40-69) -------------------------------------------------------------------------
def alteration(image, width):
    """(inds, vals) of source.py:46-60 for an overlay image array (H, W, 1..4 channels)."""
    image = np.asarray(image)
    while image.shape[2] < 4:
        image = np.append(image, np.ones((*image.shape[:2], 1), dtype=np.uint8), 2)
    ii, jj = np.nonzero(image[:, :, 3] != 0)
    k = (ii.astype(np.int64) * width + jj) * 3
    return np.stack([k, k + 1, k + 2], axis=1).reshape(-1), image[ii, jj, :3].reshape(-1)


def alteration_loop(image, width):
    """The reference's own loop, statement for statement (for small overlays: the tests compare the two forms)."""
    image = np.asarray(image)
    while image.shape[2] < 4:
        image = np.append(image, np.ones((*image.shape[:2], 1), dtype=np.uint8), 2)
    inds, vals = [], []
    for i in range(image.shape[0]):
        for j in range(image.shape[1]):
            if image[i, j, 3] == 0:
                continue
            k = (i * width + j) * 3
            inds += [k, k + 1, k + 2]
            vals += image[i, j, :3].tolist()
    return inds, vals


def alter(array, overlay):
    """source.py:65-69 on a copy: numpy.put on the flat array, whatever the pixmap's channel count."""
    array = np.array(array)
    inds, vals = alteration(overlay, array.shape[1])
    np.put(array, inds, vals)
    return array


# ---- hand-built trees the GPU tests use -------------------------------------------------------------------------------
def full_tree(seed=0):
    """40 nodes: every slot a mix (1 triple + 3 + 9 mixes + 27 leaves), leaves of all three kinds."""
    rng = random.Random(seed)

    def leaf():
        kind = rng.choice([NODE_I, NODE_J, NODE_RGB])
        return (kind, rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1)) if kind == NODE_RGB else (kind, None, None, None)

    def mix(depth):
        return (NODE_MIX, *[(mix(depth - 1) if depth > 1 else leaf()) for _ in range(3)])
    return (NODE_TRIPLE, mix(2), mix(2), mix(2))


def leaf_tree(kinds=(NODE_I, NODE_J, NODE_RGB), rgb=(0.25, -0.5, 0.75)):
    """4 nodes: every top slot a leaf."""
    return (NODE_TRIPLE, *[(k, *rgb) if k == NODE_RGB else (k, None, None, None) for k in kinds])


# ---- what the CPU and the GPU tests share -----------------------------------------------------------------------------
def save_png(array, directory, name):
    import os

    import PIL.Image
    path = os.path.join(str(directory), name)
    PIL.Image.fromarray(np.asarray(array)).save(path)
    return path


def hip_source(P, z, tmp_path):
    """The source of module P (transflow_amd.pixmap) that a fixture tests/golden/px_*.npz describes."""
    kind, h, w, seed = str(z["kind"]), int(z["height"]), int(z["width"]), int(z["seed"])
    alt = save_png(z["overlay"], tmp_path, "overlay.png") if "overlay" in z.files else None
    if kind == "image":
        return P.HipImagePixmapSource(save_png(z["image"], tmp_path, "image.png"), alt)
    if kind == "color":
        return P.HipColorPixmapSource(w, h, str(z["color"]) or None, seed, alt)
    cls = {"gradient": P.HipGradientPixmapSource, "noise": P.HipNoisePixmapSource, "bwnoise": P.HipBwNoisePixmapSource,
           "cnoise": P.HipColoredNoisePixmapSource}[kind]
    return cls(w, h, seed, alt)
