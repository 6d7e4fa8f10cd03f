"""The cases of the PNG-encode tests and the reference's encode of each, computed once and shared by tests/test_png_encode_cpu.py and
tests/test_gpu_png_encode.py.  Every case is (image, filters); each is the smallest shape at which a rule of include/ocrvi.h, "PNG
encode", can go wrong.  The images are built here from fixed seeds; tests/golden/png_encode_cases.npz holds the SHA-256 of the reference's
file for every case, the page and the many-block case (tests/golden/make_png_encode_golden.py writes it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
import pngenc_ref  # noqa: E402
from png_cases import FILTER_PAIRS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "png_encode_cases.npz")
B = pngenc_ref.BLOCK
PAGE = "page_960x1280_rgb"
PAGE_ARGS = (7, 960, 1280, 30)          # synth.make_invoice seed, h, w, lines
BIG = "chunks_2112x2048_grey"          # 265 deflate blocks: more than one 256-block chunk of the per-page scan, the last nine stored
RUNS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517)
FIXED = ("none", "sub", "up", "average", "paeth")


def text_like(rng, h, w):
    """Paper with dark strokes: long runs and few symbols, so dynamic codes win."""
    img = np.full((h, w), 255, np.uint8)
    for _ in range(max(1, h * w // 40)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y, x:x + int(rng.integers(1, 6))] = rng.integers(0, 90)
    return img


def walk_filters(rng, w=20):
    """26 rows of RGB whose row y is cheapest under filter FILTER_PAIRS[y]: a small residual undone with that filter (tests/png_ref.py's
    unfilter), so every ordered pair of filters on neighbouring rows occurs."""
    rows = np.zeros((len(FILTER_PAIRS), 1 + 3 * w), np.uint8)
    rows[:, 0] = FILTER_PAIRS
    rows[:, 1:] = rng.integers(0, 2, (len(FILTER_PAIRS), 3 * w)) * rng.integers(37, 90, (len(FILTER_PAIRS), 3 * w))
    return png_ref.unfilter(rows, 3).reshape(len(FILTER_PAIRS), w, 3)


def build():
    rng = np.random.default_rng(2100)
    c = {}
    c["g_1x1"] = (np.array([[200]], np.uint8), "adaptive")
    c["rgb_1x1"] = (np.array([[[1, 128, 255]]], np.uint8), "adaptive")
    c["row_1x300"] = (text_like(rng, 1, 300), "adaptive")
    c["col_300x1"] = (text_like(rng, 300, 1), "adaptive")
    c["rgb_7x6"] = (rng.integers(0, 256, (7, 6, 3)).astype(np.uint8) // 64 * 64, "adaptive")        # 1 + row_bytes = 19
    walk = walk_filters(rng)
    for f in FIXED + ("adaptive",):
        c["walk_26x20_" + f] = (walk, f)
    c["tie_5x9"] = (np.full((5, 9), 100, np.uint8), "adaptive")      # row 0: sub ties with paeth; below: up ties with paeth at cost 0
    for n in RUNS:
        c[f"run_{n}"] = (np.array([[7] + [50] * n + [9]], np.uint8), "none")
    c["zeros_40x50"] = (np.zeros((40, 50), np.uint8), "adaptive")
    c["exact_B"] = (text_like(rng, 128, 127), "adaptive")            # 128 x 128 = B
    c["B_minus_1"] = (text_like(rng, 129, 126), "adaptive")          # 129 x 127 = B - 1
    c["B_plus_1"] = (text_like(rng, 145, 112), "adaptive")           # 145 x 113 = B + 1
    c["cross_130x127"] = (np.zeros((130, 127), np.uint8), "adaptive")        # one run over the block boundary at B
    c["noise_64x64"] = (rng.integers(0, 256, (64, 64)).astype(np.uint8), "adaptive")
    # blocks of 128 rows of 128 bytes: noise (stored), text (dynamic), noise (stored, after a block that does not end on a byte), then a
    # last block of one constant row (fixed)
    mix = np.concatenate([rng.integers(0, 256, (128, 127)), text_like(rng, 128, 127), rng.integers(0, 256, (128, 127)),
                          np.full((1, 127), 77)]).astype(np.uint8)
    c["mix_385x127"] = (mix, "none")
    # 41 literals, 30 of them above 143 (9 bits in the fixed code): 10 + 8 x 41 + 30 bits as fixed = 40 + 8 x 41 as stored, a tie
    c["tie_types_1x40"] = (np.array([[144 + k if k < 30 else 3 * k for k in range(40)]], np.uint8), "none")
    c["rgb_70x90"] = (np.repeat(text_like(rng, 70, 90)[:, :, None], 3, axis=2) ^ rng.integers(0, 2, (70, 90, 3)).astype(np.uint8), "adaptive")
    return c


CASES = build()
NAMES = list(CASES)
_REF = {}


def image(name) -> np.ndarray:
    if name == PAGE:
        from ocr_vi_invoice_amd import synth
        seed, h, w, lines = PAGE_ARGS
        return synth.make_invoice(seed, h, w, lines=lines)[0]
    if name == BIG:
        rng = np.random.default_rng(2102)
        return np.concatenate([np.tile(text_like(rng, 64, 128), (32, 16)), rng.integers(0, 256, (64, 2048)).astype(np.uint8)])
    return CASES[name][0]


def filters(name) -> str:
    return "adaptive" if name in (PAGE, BIG) else CASES[name][1]


def ref(name):
    """The reference's encode of a case, computed once; callers leave it unchanged."""
    if name not in _REF:
        _REF[name] = pngenc_ref.encode(image(name), filters(name))
    return _REF[name]


def golden():
    return np.load(GOLDEN)


def code_histograms():
    """[(label, counts uint32 [k, n], limit)]: what ocrvi_test_png_code_lengths is checked on."""
    rng = np.random.default_rng(2101)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])

    def row(n, pairs):
        r = np.zeros(n, np.uint32)
        for k, v in pairs:
            r[k] = v
        return r
    rows = [row(286, enumerate(fib[:30])),                                   # depth 29 without the limit
            row(286, [(285 - k, v) for k, v in enumerate(fib[:40])]),        # the same from the other end, deeper
            row(286, [(256, 1)]), row(286, [(0, 3)]), row(286, []),          # one symbol (the end of block / symbol 0 joins), none
            row(286, [(65, 9), (256, 1)]), row(286, [(0, 1), (1, 1)]),       # two symbols
            np.full(286, 5, np.uint32), np.arange(1, 287).astype(np.uint32),  # uniform; all used
            (rng.integers(1, 4000, 286)).astype(np.uint32)]
    for _ in range(6):
        r = rng.integers(0, 3000, 286) * (rng.random(286) < rng.random())
        rows.append(r.astype(np.uint32))
    big = np.stack(rows)
    small = [row(19, enumerate(fib[:19])), row(19, [(18, 1)]), row(19, [(0, 4), (8, 4)]), np.full(19, 2, np.uint32),
             np.arange(1, 20).astype(np.uint32), row(19, [])]
    for _ in range(6):
        small.append((rng.integers(0, 60, 19) * (rng.random(19) < 0.6)).astype(np.uint32))
    return [("literal/length", big, 15), ("code-length", np.stack(small), 7)]
