"""Generate tests/golden/jpeg_encode_cases.npz: seeded images, the bytes PIL (libjpeg-turbo) writes for them and PIL's decode of those bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_encode_golden.py

Needs PIL; the tests read the archive only.  Archive members:
  names, kinds, modes, quality the cases, in order.  kind: "pil" (image, file and decode stored) or "sha" (page-size: rebuilt from
                               synth.make_invoice, only the SHA-256 of the file stored); mode: "420", "444" or "grey"
  i_<name>                     uint8 [h, w, 3] RGB or [h, w]: the input
  j_<name>                     PIL's file: Image.fromarray(i).save(buf, "JPEG", quality=q, subsampling=2 or 0), or mode "L"
  d_<name>                     uint8 [h, w, 3]: Image.open(j).convert("RGB"), PIL's decode of its own file
  h_<name>                     uint8 [32]: SHA-256 of the file's bytes
Cases (each the smallest at which a rule of include/ocrvi.h, "JPEG encode", can go wrong): 1x1, 8x8, 16x16, 17x23 (an odd luma block column:
a dummy block on the right), 33x50 (dummy blocks on the right and at the bottom), 31x18 (chroma of 9 columns), 40x57, all in the three
modes at quality 85, and 33x50 at qualities 1, 30 and 100 as well; 48x64 noise at quality 100 (byte stuffing: at least 10 FF 00 pairs
asserted); a 32x32 one-pixel checkerboard at quality 60 and at quality 10 (only the latter has a zero run above 15: ZRL); 32x32
alternating black and white 8x8 blocks at quality 100, grey (DC category 11); a flat image (EOB only); 200x328 noise at quality 100 (more
blocks than one chunk of any per-page loop) and one synth.make_invoice page of 500 x 380 at quality 95 ("sha").  8x8, 40x57 and 200x328
are also the heights (a multiple of 8, not of 16) at which the chroma rows below the image must repeat the last down-sampled row.  Two
runs write the same bytes (fixed seeds, zip members dated 1980)."""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np
from PIL import Image

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "jpeg_encode_cases.npz")
MODES = ("420", "444", "grey")
PAGE = ("page_500x380_420_q95", 7, 500, 380, 14, 95)        # name, make_invoice seed, h, w, lines, quality


def image(seed, h, w):
    """A gradient, stripes, a dark bar and a noise patch (the picture tests/golden/make_jpeg_golden.py draws)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 37) % 256], axis=-1).astype(np.int64)
    img[:, (x[0] // 3) % 2 == 1] //= 2
    img[h // 3:h // 3 + max(h // 8, 1), :, :] = 20
    ph, pw = max(h // 2, 1), max(w // 2, 1)
    img[h - ph:, w - pw:] = rng.integers(0, 256, (ph, pw, 3))
    return img.astype(np.uint8)


def encode(img, mode, q):
    buf = io.BytesIO()
    if mode == "grey":
        assert img.ndim == 2
        Image.fromarray(img, "L").save(buf, "JPEG", quality=q)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=q, subsampling={"420": 2, "444": 0}[mode])
    return buf.getvalue()


def for_mode(img, mode):
    return np.ascontiguousarray(img[:, :, 1]) if mode == "grey" else img


def main():
    cases = []      # (name, kind, mode, quality, image)
    seed = 300
    for (h, w) in [(1, 1), (8, 8), (16, 16), (17, 23), (33, 50), (31, 18), (40, 57)]:
        for mode in MODES:
            seed += 1
            cases.append((f"s{h}x{w}_{mode}_q85", "pil", mode, 85, for_mode(image(seed, h, w), mode)))
    for q in (1, 30, 100):
        for mode in MODES:
            seed += 1
            cases.append((f"s33x50_{mode}_q{q}", "pil", mode, q, for_mode(image(seed, 33, 50), mode)))
    rng = np.random.default_rng(400)
    cases.append(("noise_48x64_420_q100", "pil", "420", 100, rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)))
    y, x = np.mgrid[0:32, 0:32]
    checker = (((x + y) % 2) * 255).astype(np.uint8)
    cases.append(("checker_32x32_420_q60", "pil", "420", 60, np.stack([checker] * 3, axis=-1)))
    cases.append(("checker_32x32_grey_q60", "pil", "grey", 60, checker))
    # at quality 60 the checkerboard's longest zero run is 10; at quality 10 coefficient 36 follows 31 zeros, which takes a ZRL
    cases.append(("checker_32x32_420_q10", "pil", "420", 10, np.stack([checker] * 3, axis=-1)))
    cases.append(("checker_32x32_grey_q10", "pil", "grey", 10, checker))
    cases.append(("blocks_32x32_grey_q100", "pil", "grey", 100, ((((x // 8) + (y // 8)) % 2) * 255).astype(np.uint8)))
    cases.append(("flat_24x40_420_q85", "pil", "420", 85, np.full((24, 40, 3), (200, 90, 30), np.uint8)))
    cases.append(("flat_24x40_grey_q85", "pil", "grey", 85, np.full((24, 40), 77, np.uint8)))
    cases.append(("noise_200x328_420_q100", "pil", "420", 100, rng.integers(0, 256, (200, 328, 3)).astype(np.uint8)))
    from ocr_vi_invoice_amd import synth
    name, pseed, ph, pw, lines, pq = PAGE
    cases.append((name, "sha", "420", pq, synth.make_invoice(pseed, ph, pw, lines=lines)[0]))

    arrays = {"names": np.array([c[0] for c in cases]), "kinds": np.array([c[1] for c in cases]), "modes": np.array([c[2] for c in cases]),
              "quality": np.array([c[3] for c in cases], np.int32)}
    for name, kind, mode, q, img in cases:
        data = encode(img, mode, q)
        arrays["h_" + name] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8)
        if kind == "pil":
            arrays["i_" + name] = img
            arrays["j_" + name] = np.frombuffer(data, np.uint8)
            arrays["d_" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        if name.startswith("noise_48x64"):
            scan = data[data.index(b"\xff\xda"):]
            assert scan.count(b"\xff\x00") >= 10, scan.count(b"\xff\x00")
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
