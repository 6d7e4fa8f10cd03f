"""``DetectionDataset`` -- the reference's detection dataloader without augmentation (src/det/dataloader.py:27-362, ``is_training=False``,
plus the threshold maps of ``is_training=True`` with ``thresh_maps=True``) on libocrvi: the batches ``validate_detection`` consumes, built
from polygon annotations.

Per batch: the polygon geometry of all its images in one host call (``ocrvi_db_target_jobs``: validity, area, perimeter, Clipper's
shrinking and dilating offset), one upload of the fill jobs, and two kernels -- ``ocrvi_db_target_maps`` (``gt``, ``mask``, ``thresh_map``,
``thresh_mask``) and ``ocrvi_resize_normalize_pad_pages`` (``image``).  JPEG and PNG files are decoded on the device by ``pipeline.imdecode``.
Augmentation (dataloader.py:200-234) is training and is not here.  include/ocrvi.h ("DB ground truth") states the arithmetic."""
from __future__ import annotations

import ctypes as C
import glob
import json
import os
import re
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import pipeline

MAPS = ("gt", "mask", "thresh_map", "thresh_mask")
# what cv2.imread decodes and this library does not: such a file must not be blanked silently
_FOREIGN = ((b"BM", "BMP"), (b"II*\x00", "TIFF"), (b"MM\x00*", "TIFF"), (b"RIFF", "WebP / RIFF"),
            (b"\x00\x00\x00\x0cjP  ", "JPEG 2000"), (b"P5", "PGM"), (b"P6", "PPM"))


def _threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def target_jobs(sizes, polygons, shrink_ratio: float = 0.4, want_thresh: bool = False, threads: Optional[int] = None,
                cap_jobs: Optional[int] = None, cap_points: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``ocrvi_db_target_jobs`` (host only, needs no GPU): ``sizes`` = [(h, w), ...], ``polygons`` = per image a list of (k, 2) float
    arrays -> (jobs int32 [n_jobs, 8] = (image, kind, p0, p1, x0, y0, x1, y1), points int32 [n_points, 2]).  The capacities are a first
    guess; when the entry reports that more room is needed the call is repeated with exactly that room."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    n = len(sizes)
    if n == 0 or n != len(polygons):
        raise ValueError(f"target_jobs: {n} sizes for {len(polygons)} polygon lists")
    flat, poly_offs, img_offs = [], [0], [0]
    for polys in polygons:
        for p in polys:
            p = np.asarray(p, dtype=np.float32)
            if p.ndim != 2 or p.shape[1] != 2:
                raise ValueError(f"target_jobs: a polygon must be a (k, 2) array, got shape {p.shape}")
            flat.append(p)
            poly_offs.append(poly_offs[-1] + len(p))
        img_offs.append(len(poly_offs) - 1)
    xy = np.ascontiguousarray(np.concatenate(flat, axis=0)) if flat else np.zeros((0, 2), np.float32)
    poly_offs, img_offs = np.asarray(poly_offs, np.int32), np.asarray(img_offs, np.int32)
    # a polygon gives at most two jobs; Clipper's round joins add vertices, so the point room is a guess the entry may correct
    cap_j = 2 * (len(poly_offs) - 1) + 1 if cap_jobs is None else cap_jobs
    cap_p = 8 * len(xy) + 256 * (len(poly_offs) - 1) + 16 if cap_points is None else cap_points
    nj, npts, over = C.c_int32(), C.c_int32(), C.c_int32()
    lib = _lib.load()
    for _ in range(2):
        jobs, points = np.empty((max(cap_j, 1), _lib.DB_TARGET_JOB), np.int32), np.empty((max(cap_p, 1), 2), np.int32)
        _lib.check(lib.ocrvi_db_target_jobs(sizes.ctypes.data, xy.ctypes.data if len(xy) else None, poly_offs.ctypes.data, img_offs.ctypes.data, n,
                                            float(shrink_ratio), int(bool(want_thresh)), jobs.ctypes.data, cap_j, points.ctypes.data, cap_p,
                                            C.byref(nj), C.byref(npts), C.byref(over), threads or _threads()))
        if not over.value:
            return jobs[:nj.value], points[:npts.value]
        cap_j, cap_p = max(cap_j, nj.value), max(cap_p, npts.value)
    raise RuntimeError("ocrvi_db_target_jobs asked for more room twice")


def resize_sizes(h: int, w: int, S: int) -> Tuple[int, int]:
    """(new_h, new_w) of _resize_pad (dataloader.py:242-244), in Python's double arithmetic."""
    scale = S / max(h, w)
    return int(h * scale), int(w * scale)


class DetectionDataset:
    """``DetectionDataset(data_dir)`` reads the reference's layout: the sorted ``*.json`` files of ``data_dir``, each with
    ``annotations[].polygon`` (polygons of at least 3 points are kept) and its image beside it (``.jpg``, then ``.png``).
    ``DetectionDataset(samples=[(image, polygons), ...])`` takes images directly: a uint8 HxWx3 RGB array or tensor, or the bytes of a
    baseline JPEG file or of a PNG file.

    ``len(ds)``, ``ds[i]`` (the reference's dict of ``image`` [3,S,S] and ``gt``, ``mask``, ``thresh_map``, ``thresh_mask`` [1,S,S], float32
    on ``device``) and ``ds.batches(batch_size)`` (dicts of [B,...] tensors, in order, the last one short).  ``thresh_maps=True`` fills the
    threshold maps as ``is_training=True`` does; the reference's map equals ``thresh_max`` over the whole dilated polygon (include/ocrvi.h),
    so ``thresh_min`` is kept for the signature only.

    A sample the reference would replace by ``_blank_sample()`` -- an unreadable image, a broken annotation, a side that resizes to 0 --
    yields that blank sample and is recorded in ``ds.blank`` as (index, reason).  A file cv2 would read and this library cannot (BMP,
    progressive JPEG, an interlaced PNG, ...) and a JPEG or PNG file the library finds corrupt raise ValueError naming it."""

    def __init__(self, data_dir: Optional[str] = None, samples: Optional[Sequence] = None, image_size: int = 640, shrink_ratio: float = 0.4,
                 thresh_min: float = 0.3, thresh_max: float = 0.7, thresh_maps: bool = False, device: str = "cuda:0"):
        if (data_dir is None) == (samples is None):
            raise ValueError("DetectionDataset: give either data_dir or samples")
        if not 1 <= int(image_size) <= _lib.DB_TARGET_MAX_SIDE:
            raise ValueError(f"DetectionDataset: image_size {image_size} outside 1 .. {_lib.DB_TARGET_MAX_SIDE}")
        if not 0.0 < shrink_ratio < 1.0:
            raise ValueError(f"DetectionDataset: shrink_ratio {shrink_ratio} outside (0, 1)")
        if not thresh_max > 0.0:
            raise ValueError("DetectionDataset: thresh_max must be positive (the reference's map update is `thresh_vals > thresh_map`)")
        self.image_size, self.shrink_ratio = int(image_size), float(shrink_ratio)
        self.thresh_min, self.thresh_max, self.thresh_maps = float(thresh_min), float(thresh_max), bool(thresh_maps)
        self.device = torch.device(device)
        self.data_dir = data_dir
        self.samples = sorted(glob.glob(os.path.join(data_dir, "*.json"))) if data_dir is not None else list(samples)
        self.blank: List[Tuple[int, str]] = []

    def __len__(self) -> int:
        return len(self.samples)

    # ---------------------------------------------------------------------------------------------- loading
    def _note_blank(self, idx: int, reason: str) -> None:
        if all(i != idx for i, _ in self.blank):
            self.blank.append((idx, reason))

    @staticmethod
    def _polygons(raw) -> List[np.ndarray]:
        out = []
        for p in raw:
            a = np.array(p, dtype=np.float32)
            if len(a) >= 3:                                   # dataloader.py:320
                if a.ndim != 2 or a.shape[1] != 2 or not np.isfinite(a).all():
                    raise ValueError(f"polygon of shape {a.shape} is not a finite (k, 2) array")
                out.append(a)
        return out

    def _read_file(self, json_path: str):
        """-> (path, JPEG or PNG bytes, polygons); an Exception here is what the reference turns into a blank sample, a ValueError from
        ``_foreign`` is not."""
        with open(json_path, "r", encoding="utf-8") as f:
            annotation = json.load(f)
        data = None
        for ext in (".jpg", ".png"):                          # dataloader.py:307-311
            path = json_path[:-len(".json")] + ext
            try:
                with open(path, "rb") as f:
                    data = f.read()
            except OSError:
                continue
            for magic, fmt in _FOREIGN:
                if data.startswith(magic):
                    raise _Foreign(f"{path}: a {fmt} file; only baseline JPEG and PNG are decoded here")
            if data.startswith(b"\xff\xd8") or data.startswith(pipeline.PNG_SIGNATURE):
                return path, data, self._polygons(a["polygon"] for a in annotation.get("annotations", []))
            data = None                                       # neither cv2 nor this library reads it: try the next name
        raise OSError(f"Cannot read image for {os.path.basename(json_path)}")

    def _load(self, idx: int):
        """-> (image source, polygons, (h, w, new_h, new_w), name) or None for a blank sample.  The source is a device/host uint8 tensor or
        the bytes of a JPEG or PNG file."""
        item = self.samples[idx]
        name = f"sample {idx}"
        try:
            if self.data_dir is not None:
                name, image, polygons = self._read_file(item)
            else:
                image, polygons = item[0], self._polygons(item[1])
        except _Foreign as e:
            raise ValueError(str(e)) from None
        except Exception as e:                                # dataloader.py:281-286
            self._note_blank(idx, f"{type(e).__name__}: {e}")
            return None
        if isinstance(image, pipeline.IMAGE_BYTES):            # ValueError naming the file for what the library refuses
            info = (pipeline.png_info_struct if pipeline.is_png(image) else pipeline.jpeg_info_struct)(image, name)
            h, w = info.out_height, info.out_width
        else:
            if isinstance(image, np.ndarray):
                image = torch.from_numpy(np.ascontiguousarray(image))
            if not (isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3):
                raise ValueError(f"{name}: an image is a uint8 HxWx3 array or tensor, or JPEG or PNG bytes")
            h, w = int(image.shape[0]), int(image.shape[1])
        if h < 1 or w < 1:
            self._note_blank(idx, f"empty image ({h} x {w})")
            return None
        if max(h, w) > _lib.DB_TARGET_MAX_SIDE:
            raise ValueError(f"{name}: {h} x {w} exceeds the largest side {_lib.DB_TARGET_MAX_SIDE}")
        new_h, new_w = resize_sizes(h, w, self.image_size)
        if new_h < 1 or new_w < 1:                            # cv2.resize raises on an empty destination
            self._note_blank(idx, f"{h} x {w} resizes to {new_h} x {new_w}")
            return None
        return image, polygons, (h, w, new_h, new_w), name

    # ---------------------------------------------------------------------------------------------- batches
    def _batch(self, indices: Sequence[int]) -> Dict[str, torch.Tensor]:
        dev, S, n = self.device, self.image_size, len(indices)
        loaded = [self._load(i) for i in indices]
        rows = np.zeros((n, 4), np.int32)
        for k, item in enumerate(loaded):
            if item is not None:
                rows[k] = item[2]
        sizes = np.maximum(rows[:, :2], 1)                    # a blank sample has no polygons; its size is not read
        jobs, points = target_jobs(sizes, [item[1] if item is not None else [] for item in loaded], self.shrink_ratio, self.thresh_maps)
        with torch.cuda.device(dev):
            files = [k for k, item in enumerate(loaded) if item is not None and isinstance(item[0], pipeline.IMAGE_BYTES)]
            pages: List[Optional[torch.Tensor]] = [None] * n
            if files:
                try:
                    decoded = pipeline.imdecode([loaded[k][0] for k in files], str(dev))
                except ValueError as e:                       # a corrupt file, found while decoding: named by its file, not its index
                    m = re.match(r"imdecode: file (\d+): (.*)", str(e), re.S)
                    if m is None:
                        raise
                    raise ValueError(f"{loaded[files[int(m.group(1))]][3]}: {m.group(2)}") from None
                for k, page in zip(files, decoded):
                    pages[k] = page
            for k, item in enumerate(loaded):
                if item is not None and pages[k] is None:
                    pages[k] = item[0].to(dev, non_blocking=True).contiguous()
            # one upload: the page table (int64), then rows, jobs and points (int32)
            table = np.zeros((n, _lib.PAGE_ENTRY), np.int64)
            for k, page in enumerate(pages):
                if page is not None:
                    table[k, :3] = (page.data_ptr(), rows[k, 0], rows[k, 1])
            parts = [table.view(np.int32).ravel(), rows.ravel(), jobs.ravel(), points.ravel()]
            offs = np.cumsum([0] + [p.size for p in parts])
            host = torch.empty(int(offs[-1]), dtype=torch.int32).pin_memory()
            host.numpy()[:] = np.concatenate(parts)
            d = host.to(dev, non_blocking=True)
            base = d.data_ptr()
            out = {"image": torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)}
            out.update({k: torch.empty((n, 1, S, S), dtype=torch.float32, device=dev) for k in MAPS})
            lib, devi = _lib.load(), pipeline._dev_index(dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.ocrvi_db_target_maps(devi, base + 4 * int(offs[2]), len(jobs), base + 4 * int(offs[3]), len(points), base + 4 * int(offs[1]),
                                                n, S, self.thresh_max, *[out[k].data_ptr() for k in MAPS], stream))
            _lib.check(lib.ocrvi_resize_normalize_pad_pages(devi, base, base + 4 * int(offs[1]), n, S, out["image"].data_ptr(), stream))
        return out      # (the table, the jobs and the pages were allocated on the stream that reads them: freeing them here is ordered)

    def batches(self, batch_size: int) -> Iterator[Dict[str, torch.Tensor]]:
        if batch_size < 1:
            raise ValueError("batches: batch_size must be at least 1")
        for i0 in range(0, len(self), batch_size):
            yield self._batch(range(i0, min(i0 + batch_size, len(self))))

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        if not -len(self) <= idx < len(self):
            raise IndexError(idx)
        return {k: v[0] for k, v in self._batch([idx % len(self)]).items()}


class _Foreign(Exception):
    """An image file of a format cv2 decodes and this library does not."""
