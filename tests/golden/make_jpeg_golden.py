"""Generate tests/golden/jpeg_cases.npz: seeded images encoded with PIL (libjpeg-turbo) and PIL's own decode of each file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_golden.py

Needs PIL; the tests read the archive only.  Every image has structure (a gradient, stripes, a dark bar) plus a noise patch, so that every
coefficient position occurs.  Archive members:
  names, kinds                 the cases, in order.  kind: "pil" (PIL's RGB stored, the claim is equality with it), "sha" (page-size: only
                               the SHA-256 of PIL's RGB bytes), "ref" (streams no encoder produces: pinned to tests/jpeg_ref.py only),
                               "bad" (files the library refuses, naming the feature)
  j_<name>                     the file's bytes
  p_<name>                     uint8 [h, w, 3]: Image.open(...).convert("RGB"), after ImageOps.exif_transpose for the orientation cases
  h_<name>                     uint8 [32]: SHA-256 of that array's bytes
Cases: h x w in 1x1 7x9 8x8 16x16 17x33 33x17 8x40 97x131 crossed with 4:4:4 / 4:2:2 / 4:2:0 at quality 85; 33x17 and 97x131 at quality 30 and
100; 3x4, 5x3 and 2x2 (chroma planes of one or two samples, where the library replicates instead of filtering); restart intervals of 1 MCU, 3
MCUs and one MCU row on 33x17 and 97x131; a grey file; optimize=True; 16-bit quantisation tables (the DQT of a quality-100 file rewritten
with two bytes per entry: the values and therefore PIL's output are unchanged); the eight EXIF orientations on 33x17 4:2:0 (odd values in
a big-endian, even values in a little-endian TIFF header); every quantisation entry patched to 255 ("ref"); a progressive and a CMYK file
("bad"); one synth.make_invoice page of 500 x 380 at quality 85 4:2:0 and two smaller ones, 420 x 320 (4:2:0) and 320 x 420 (4:2:2) ("sha").
Two runs write the same bytes (fixed seeds, zip members dated 1980)."""
import hashlib
import io
import os
import struct
import sys
import zipfile

import numpy as np
from PIL import Image, ImageOps

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "jpeg_cases.npz")
SUB = {"444": 0, "422": 1, "420": 2}


def image(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 37) % 256], axis=-1).astype(np.int64)
    img[:, (x[0] // 3) % 2 == 1] //= 2                       # stripes
    img[h // 3:h // 3 + max(h // 8, 1), :, :] = 20           # a dark bar
    ph, pw = max(h // 2, 1), max(w // 2, 1)
    img[h - ph:, w - pw:] = rng.integers(0, 256, (ph, pw, 3))  # the noise patch
    return img.astype(np.uint8)


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def segments(data):
    """(marker, start, end) of every segment up to SOS."""
    p, out = 2, []
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + ln))
        if m == 0xDA:
            return out
        p += 2 + ln


def dqt_16bit(data):
    out, last = bytearray(data[:2]), 2
    for m, a, b in segments(data):
        out += data[last:a]
        last = b
        if m != 0xDB:
            out += data[a:b]
            continue
        body, q, new = data[a + 4:b], 0, bytearray()
        while q < len(body):
            assert body[q] >> 4 == 0
            new += bytes([0x10 | body[q]]) + b"".join(struct.pack(">H", v) for v in body[q + 1:q + 65])
            q += 65
        out += b"\xff\xdb" + struct.pack(">H", len(new) + 2) + new
    return bytes(out + data[last:])


def dqt_255(data):
    out = bytearray(data)
    for m, a, b in segments(data):
        if m == 0xDB:
            q = a + 4
            while q < b:
                out[q + 1:q + 65] = b"\xff" * 64
                q += 65
    return bytes(out)


def with_exif(data, k):
    e = ">" if k % 2 else "<"
    tiff = (b"MM\0*" if k % 2 else b"II*\0") + struct.pack(e + "I", 8) + struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, k, 0) + \
        struct.pack(e + "I", 0)
    seg = b"Exif\0\0" + tiff
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(seg) + 2) + seg + data[2:]


def main():
    cases = []      # (name, kind, bytes)
    sizes = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (33, 17), (8, 40), (97, 131)]
    seed = 100
    for (h, w) in sizes:
        for s in SUB:
            seed += 1
            cases.append((f"s{h}x{w}_{s}_q85", "pil", encode(image(seed, h, w), quality=85, subsampling=SUB[s])))
    for (h, w) in [(33, 17), (97, 131)]:
        for q in (30, 100):
            for s in SUB:
                seed += 1
                cases.append((f"s{h}x{w}_{s}_q{q}", "pil", encode(image(seed, h, w), quality=q, subsampling=SUB[s])))
    for (h, w) in [(3, 4), (5, 3), (2, 2)]:
        for s in ("422", "420"):
            seed += 1
            cases.append((f"s{h}x{w}_{s}_q85", "pil", encode(image(seed, h, w), quality=85, subsampling=SUB[s])))
    for (h, w) in [(33, 17), (97, 131)]:
        seed += 1
        img = image(seed, h, w)
        cases.append((f"rst1_{h}x{w}", "pil", encode(img, quality=85, subsampling=2, restart_marker_blocks=1)))
        cases.append((f"rst3_{h}x{w}", "pil", encode(img, quality=85, subsampling=2, restart_marker_blocks=3)))
        cases.append((f"rstrow_{h}x{w}", "pil", encode(img, quality=85, subsampling=2, restart_marker_rows=1)))
    cases.append(("grey_33x17", "pil", encode(image(201, 33, 17)[:, :, 0], quality=85)))
    cases.append(("optimize_97x131", "pil", encode(image(202, 97, 131), quality=85, subsampling=2, optimize=True)))
    cases.append(("q16_33x17", "pil", dqt_16bit(encode(image(203, 33, 17), quality=100, subsampling=2))))
    base = encode(image(204, 33, 17), quality=85, subsampling=2)
    for k in range(1, 9):
        cases.append((f"orient{k}_33x17", "pil", with_exif(base, k)))
    cases.append(("oor_33x17", "ref", dqt_255(encode(image(205, 33, 17), quality=100, subsampling=2))))
    cases.append(("progressive_33x17", "bad", encode(image(206, 33, 17), quality=85, progressive=True)))
    buf = io.BytesIO()
    Image.fromarray(image(207, 16, 16)).convert("CMYK").save(buf, "JPEG", quality=85)
    cases.append(("cmyk_16x16", "bad", buf.getvalue()))
    from ocr_vi_invoice_amd import synth
    page, _ = synth.make_invoice(7, 500, 380, lines=14)
    cases.append(("page_500x380", "sha", encode(page, quality=85, subsampling=2)))
    # two more invoices for the engine test (tests/test_gpu_jpeg_engine.py)
    cases.append(("inv1_420x320", "sha", encode(synth.make_invoice(8, 420, 320, lines=10)[0], quality=85, subsampling=2)))
    cases.append(("inv2_320x420", "sha", encode(synth.make_invoice(9, 320, 420, lines=8)[0], quality=85, subsampling=1)))

    arrays = {"names": np.array([c[0] for c in cases]), "kinds": np.array([c[1] for c in cases])}
    for name, kind, data in cases:
        arrays["j_" + name] = np.frombuffer(data, np.uint8)
        if kind in ("pil", "sha"):
            im = Image.open(io.BytesIO(data))
            rgb = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
            arrays["h_" + name] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).digest(), np.uint8)
            if kind == "pil":
                arrays["p_" + name] = rgb
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
