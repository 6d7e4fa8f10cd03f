"""Generate tests/golden/png_encode_cases.npz: the SHA-256 of the file tests/pngenc_ref.py writes for every case of
tests/pngenc_cases.py, for the page-sized case (one synth.make_invoice page of 960 x 1280, RGB, adaptive filters) and for the
many-block case (2112 x 2048 grey, 265 deflate blocks).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_png_encode_golden.py

Needs numpy only.  Before a digest is stored the file is checked the ways the tests check it: its IDAT inflates under zlib to the
reference's filtered stream, and tests/png_ref.py decodes it to the input.  Archive members:
  names        the cases, in order, then the page and the many-block case
  h_<name>     uint8 [32]: SHA-256 of the file's bytes
  n_<name>     int64: the file's bytes
Two runs write the same bytes (fixed seeds, zip members dated 1980)."""
import hashlib
import io
import os
import sys
import zipfile
import zlib

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import png_ref  # noqa: E402
import pngenc_cases as cases  # noqa: E402


def main():
    names = cases.NAMES + [cases.PAGE, cases.BIG]
    arrays = {"names": np.array(names)}
    for name in names:
        e = cases.ref(name)
        img = cases.image(name)
        idat = b"".join(b for t, b in png_ref.chunks(e.data) if t == b"IDAT")
        assert zlib.decompress(idat) == e.stream.tobytes(), name
        want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
        assert np.array_equal(png_ref.decode(e.data), want), name
        arrays["h_" + name] = np.frombuffer(hashlib.sha256(e.data).digest(), np.uint8)
        arrays["n_" + name] = np.int64(len(e.data))
    with zipfile.ZipFile(cases.GOLDEN, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(f"{cases.GOLDEN}: {len(names)} cases, {os.path.getsize(cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
