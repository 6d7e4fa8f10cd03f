"""Generate tests/golden/png_cases.npz: PNG files and PIL's own decode of each.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_png_golden.py

Needs PIL; the package and the tests read the archive only.  Archive members:
  names, kinds                 the cases, in order.  kind: "pil" (PIL's RGB stored, the claim is equality with it), "sha" (page-size: only
                               the SHA-256 of PIL's RGB bytes), "ref" (where PIL is not the claim: pinned to tests/png_ref.py only)
  f_<name>                     the file's bytes
  p_<name>                     uint8 [h, w, 3]: Image.open(...).convert("RGB")
  h_<name>                     uint8 [32]: SHA-256 of that array's bytes
Cases: every legal pair of colour type and bit depth, 23 x 19 random samples with the rows' filters cycling through all 25 ordered pairs,
written by tests/png_cases.py (t<colour>_d<depth>; 16-bit grey is "ref": PIL maps it differently); a palette file whose indices run past
its PLTE ("ref"); files written by PIL's own encoder, modes 1, L, P, RGB, RGBA and LA, optimize on and off (pil_<mode>_<opt>); an RGBA
file with gAMA, tEXt and tIME chunks around its IDAT (skipped); one synth.make_invoice page of 960 x 1280 as an 8-bit
grey file ("sha") and two smaller invoices, RGB 420 x 320 and bilevel 320 x 420, for the engine test ("sha").
Two runs write the same bytes (fixed seeds, zip members dated 1980)."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "png_cases.npz")


def image(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 37) % 256], axis=-1).astype(np.int64)
    img[:, (x[0] // 3) % 2 == 1] //= 2                       # stripes
    img[h // 3:h // 3 + max(h // 8, 1), :, :] = 20           # a dark bar
    ph, pw = max(h // 2, 1), max(w // 2, 1)
    img[h - ph:, w - pw:] = rng.integers(0, 256, (ph, pw, 3))  # the noise patch
    return img.astype(np.uint8)


def pil_png(im, **kw):
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


def main():
    import png_cases as C
    from ocr_vi_invoice_amd import synth
    cases = []      # (name, kind, bytes)
    rng = np.random.default_rng(20)
    h, w = 23, 19
    for colour, depth in C.PAIRS:
        samples = C.random_samples(rng, h, w, colour, depth)
        palette = rng.integers(0, 256, (1 << depth, 3)).astype(np.uint8) if colour == 3 else None
        filters = [C.FILTER_PAIRS[(y + colour + depth) % 25] for y in range(h)]
        cases.append((f"t{colour}_d{depth}", "ref" if (colour, depth) == (0, 16) else "pil", C.write_png(samples, colour, depth, filters, palette)))
    samples = C.random_samples(rng, 9, 14, 3, 4)             # indices 0 .. 15, PLTE of 5 entries
    cases.append(("beyond_plte", "ref", C.write_png(samples, 3, 4, [4] * 9, rng.integers(0, 256, (5, 3)).astype(np.uint8))))
    rgb = Image.fromarray(image(301, 45, 52))
    alpha = Image.fromarray(image(302, 45, 52)[:, :, 1])
    modes = {"1": rgb.convert("1"), "L": rgb.convert("L"), "P": rgb.convert("P", palette=Image.ADAPTIVE, colors=40), "RGB": rgb,
             "RGBA": Image.merge("RGBA", (*rgb.split(), alpha)), "LA": Image.merge("LA", (rgb.convert("L"), alpha))}
    for mode, im in modes.items():
        for opt in (False, True):
            cases.append((f"pil_{mode}_{'opt' if opt else 'std'}", "pil", pil_png(im, optimize=opt)))
    extra = C.chunk(b"gAMA", (45455).to_bytes(4, "big")) + C.chunk(b"tEXt", b"Comment\0skipped")
    samples = C.random_samples(rng, 12, 10, 6, 8)
    cases.append(("ancillary_rgba", "pil", C.write_png(samples, 6, 8, [3] * 12, before_idat=extra, after_idat=C.chunk(b"tIME", bytes(7)))))
    page = synth.make_invoice(7, 960, 1280, lines=30)[0]
    cases.append(("page_960x1280", "sha", pil_png(Image.fromarray(page[:, :, 0] // 16 * 17), optimize=True)))
    cases.append(("inv1_420x320", "sha", pil_png(Image.fromarray(synth.make_invoice(8, 420, 320, lines=10)[0] // 32 * 36))))
    cases.append(("inv2_320x420", "sha", pil_png(Image.fromarray(synth.make_invoice(9, 320, 420, lines=8)[0][:, :, 0] > 128))))

    arrays = {"names": np.array([c[0] for c in cases]), "kinds": np.array([c[1] for c in cases])}
    for name, kind, data in cases:
        arrays["f_" + name] = np.frombuffer(data, np.uint8)
        if kind in ("pil", "sha"):
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
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
