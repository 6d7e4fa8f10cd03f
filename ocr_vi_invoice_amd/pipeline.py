"""Host-side mirror of the reference pipeline's helpers (src/pipeline/pipeline2.py) on top of libocrvi.

Same names and argument meaning as the reference for the pieces either side of the two models:
``load_detection_model`` (:43), ``load_recognition_model`` (:72), ``preprocess_for_recognition`` (:92), ``recognize_text`` (:131),
``recognize_text_batch`` (:144), ``resize_image_for_det`` (:33), ``crop_image`` (src/det/test.py:123) plus ``normalize_for_det`` (the
inline code at :312-314), ``rescale_boxes`` (:324-328) and ``detect_and_recognize`` (steps 2-3 of the per-image loop, :306-352), and the geometric half of step 1
(``four_point_transform``, ``preprocess_image``: src/preprocess/scanner.py:29-53,168-196 with the corners supplied by the caller) and
its enhancement half (``enhance_document``, scanner.py:55-76); ``draw_boxes_with_text`` (:173) and, for the ``--save_result`` branch
(:358-360 + :397-400), ``save_result``.
Image resizing and crop pre-processing run on the GPU (ocrvi_crop_resize_normalize / ocrvi_normalize_u8).
File I/O -- ``imdecode`` / ``imread``, ``imencode*`` / ``imwrite``, the JPEG and PNG wrappers and the encode jobs -- lives in ``codec`` and
is re-exported here under the same names.

``DBPostProcessor`` (src/det/test.py:46-106) is the host C++ implementation behind ``ocrvi_db_postprocess``; like the reference's, it works on
the probability map after the device->host copy.  cv2 / pyclipper / shapely are absent from the build container, so its agreement with
those libraries is unpinned; it is checked bit-for-bit against the independent statement in oracle/dbpost_cpu.py.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import ctypes

import numpy as np
import torch

from . import _lib
from .codec import (IMAGE_BYTES, IMWRITE_FORMATS, JPEG_BYTES, JPEG_SUBSAMPLINGS, PNG_ENC_REGIONS, PNG_FILTERS, PNG_SIGNATURE, JpegEncodeJob,
                    PngEncodeJob, _check_format, _dev_index, host_pool, imdecode, imencode, imencode_pages, imencode_png, imencode_png_pages,
                    imread, imwrite, is_png, jpeg_encode_header, jpeg_encode_sizes, jpeg_info, jpeg_info_struct, jpeg_parse, jpeg_parse_into,
                    jpeg_quant_tables, jpeg_table_entry, png_encode_sizes, png_info, png_info_struct, png_parse, png_parse_into, png_plan,
                    png_table_entry)
from .det import DBNetPP
from .rec import Hypothesis, Recognition, SVTRv2, check_beam, check_lm


def _numpy_data_globals():
    """Data-only numpy reconstructors a reference-trained checkpoint carries next to ``model_state_dict``: the trainers store
    ``best_f1`` / ``best_acc`` and ``val_metrics`` as numpy scalars (src/det/val.py:111-115 -> src/det/train.py:266-272,
    src/rec2/train.py:237-260).  Allow-listing them keeps ``weights_only=True`` (nothing in the file is executed)."""
    allow = [np.dtype]
    try:
        from numpy._core.multiarray import scalar
    except ImportError:  # numpy < 2
        from numpy.core.multiarray import scalar
    allow.append(scalar)
    for name in ("Float64DType", "Float32DType", "Float16DType", "Int64DType", "Int32DType", "BoolDType", "UInt8DType"):
        t = getattr(getattr(np, "dtypes", None), name, None)
        if t is not None:
            allow.append(t)
    return allow


def load_checkpoint(model_path: str):
    """torch.load of a reference checkpoint file with the weights-only unpickler; returns whatever the file holds (a wrapped dict with
    ``model_state_dict`` or a bare state_dict -- ``weights.unwrap_checkpoint`` takes either, pipeline2.py:46-52,75-80)."""
    with torch.serialization.safe_globals(_numpy_data_globals()):
        return torch.load(model_path, map_location="cpu", weights_only=True)


def load_detection_model(model_path: str, device: str = "cuda:0", dtype: str = "f32") -> DBNetPP:
    """pipeline2.py:43-67.  The checkpoint is read with ``weights_only=True`` (nothing in the file is executed)."""
    return DBNetPP(pretrained=False, state_dict=load_checkpoint(model_path), device=device, dtype=dtype)


def load_recognition_model(model_path: str, device: str = "cuda:0", variant: str = "base", dtype: str = "f32") -> SVTRv2:
    """pipeline2.py:72-89."""
    return SVTRv2(variant=variant, in_channels=3, state_dict=load_checkpoint(model_path), device=device, dtype=dtype)


def resize_image_for_det(image, image_size: int = 640):
    """pipeline2.py:33-40: scale the longer side to ``image_size``, round both sides to multiples of 32, cv2.resize (bilinear).
    ``image``: uint8 HWC numpy array or device tensor.  Returns (resized uint8 HWC device tensor, (scale_h, scale_w))."""
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    img = img.cuda().contiguous() if not img.is_cuda else img.contiguous()
    h, w = img.shape[:2]
    scale = image_size / max(h, w)
    new_h = int(np.round(h * scale / 32) * 32)
    new_w = int(np.round(w * scale / 32) * 32)
    out = torch.empty((new_h, new_w, 3), dtype=torch.uint8, device=img.device)
    stream = torch.cuda.current_stream(img.device).cuda_stream
    _lib.check(_lib.load().ocrvi_resize_u8(_dev_index(img.device), img.data_ptr(), h, w, out.data_ptr(), new_h, new_w, stream))
    return out, (new_h / h, new_w / w)


def normalize_for_det(images_u8: torch.Tensor) -> torch.Tensor:
    """uint8 HWC [N,H,W,3] on the device -> float32 NCHW, exactly the arithmetic of pipeline2.py:312-314."""
    if images_u8.dim() == 3:
        images_u8 = images_u8[None]
    images_u8 = images_u8.contiguous()
    N, H, W, C = images_u8.shape
    assert C == 3 and images_u8.dtype == torch.uint8 and images_u8.is_cuda
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=images_u8.device)
    stream = torch.cuda.current_stream(images_u8.device).cuda_stream
    _lib.check(_lib.load().ocrvi_normalize_u8(_dev_index(images_u8.device), images_u8.data_ptr(), N, H, W, out.data_ptr(), stream))
    return out


class DBPostProcessor:
    """src/det/test.py:44-106: probability map -> unclipped text polygons + scores.  Same constructor, attributes and call signature."""

    def __init__(self, thresh=0.3, box_thresh=0.6, max_candidates=1000, unclip_ratio=1.5):
        self.thresh = thresh
        self.box_thresh = box_thresh
        self.max_candidates = max_candidates
        self.unclip_ratio = unclip_ratio
        self.min_size = 3
        self.min_area = 10

    def __call__(self, pred, is_output_polygon=False):
        """pred: (1, H, W) float array or tensor (a device tensor is copied to the host, as pipeline2.py:320 does).
        Returns (boxes, scores): boxes[i] is an (n_i, 2) int64 array of polygon vertices, scores[i] a float."""
        if isinstance(pred, torch.Tensor):
            pred = pred.detach().float().cpu().numpy()
        pred = np.asarray(pred)
        if pred.ndim == 3:
            pred = pred[0]
        if pred.ndim != 2:
            raise ValueError(f"DBPostProcessor expects (1, H, W) or (H, W), got shape {pred.shape}")
        prob = np.ascontiguousarray(pred, dtype=np.float32)
        H, W = prob.shape
        lib = _lib.load()
        cap_boxes = max(int(self.max_candidates), 1)
        cap_points = 4 * (H + W) + 4096
        while True:
            points = np.empty((cap_points, 2), np.int32)
            offs = np.empty(cap_boxes + 1, np.int32)
            scores = np.empty(cap_boxes, np.float32)
            n = ctypes.c_int32(0)
            rc = lib.ocrvi_db_postprocess(prob.ctypes.data, H, W, float(self.thresh), float(self.box_thresh), int(self.max_candidates),
                                          float(self.unclip_ratio), float(self.min_area), points.ctypes.data, cap_points, offs.ctypes.data,
                                          scores.ctypes.data, cap_boxes, ctypes.byref(n))
            if rc == -3 and cap_points < (1 << 28):
                cap_points *= 4          # more polygon vertices than guessed: retry with room
                continue
            _lib.check(rc)
            break
        boxes = [points[offs[i]:offs[i + 1]].astype(np.int64) for i in range(n.value)]
        return boxes, [float(v) for v in scores[:n.value]]


def db_boxes_batch(prob_maps, post_processor: "DBPostProcessor", scale_w: float = 1.0, scale_h: float = 1.0, orig_hw: Tuple[int, int] = None,
                   page_base: int = 0, threads: int = 8, cap_per_page: int = None, out=None):
    """The host middle of pipeline2.py:320-343 for a batch of pages, in one GIL-free call: ``post_processor`` on each map ->
    ``rescale_boxes`` -> ``crop_rect``.  ``prob_maps``: float32 [n,H,W] host array (numpy, or a CPU/pinned torch tensor).
    Returns (rects int32 [total,5] = (page, x, y, w, h) in page order, counts int32 [n], scores float32 [total])."""
    if isinstance(prob_maps, torch.Tensor):
        assert not prob_maps.is_cuda and prob_maps.dtype == torch.float32 and prob_maps.is_contiguous()
        n, H, W = prob_maps.shape[-3:] if prob_maps.dim() >= 3 else (1,) + tuple(prob_maps.shape)
        ptr = prob_maps.data_ptr()
    else:
        prob_maps = np.ascontiguousarray(prob_maps, dtype=np.float32)
        if prob_maps.ndim == 2:
            prob_maps = prob_maps[None]
        n, H, W = prob_maps.shape
        ptr = prob_maps.ctypes.data
    oh, ow = orig_hw if orig_hw is not None else (H, W)
    cap = int(cap_per_page or post_processor.max_candidates)
    if out is None:
        out = (np.empty((n, cap, 5), np.int32), np.empty((n, cap), np.float32), np.empty(n, np.int32))
    rects, scores, counts = out
    _lib.check(_lib.load().ocrvi_db_boxes_batch(ptr, n, H, W, float(post_processor.thresh), float(post_processor.box_thresh),
                                                int(post_processor.max_candidates), float(post_processor.unclip_ratio),
                                                float(post_processor.min_area), float(scale_w), float(scale_h), int(oh), int(ow), int(page_base),
                                                rects.ctypes.data, scores.ctypes.data, cap, counts.ctypes.data, int(threads)))
    keep = [rects[i, :counts[i]] for i in range(n)]
    return (np.concatenate(keep, 0) if keep else np.empty((0, 5), np.int32)), counts[:n].copy(), \
        np.concatenate([scores[i, :counts[i]] for i in range(n)], 0)



def db_boxes_pages(prob_maps, post_processor: "DBPostProcessor", scales, orig_sizes, page_ids=None, threads: int = 8, cap_points: int = None,
                   cap_per_page: int = None):
    """``db_boxes_batch`` for maps of one shape whose pages have their own scale and original size (``ocrvi_db_boxes_pages``): for page p,
    ``post_processor`` on its map -> ``rescale_boxes`` with ``scales[p] = (scale_h, scale_w)`` -> ``crop_rect`` in ``orig_sizes[p] = (h, w)``.
    ``prob_maps``: float32 [n,H,W] host array (numpy, or a CPU/pinned torch tensor).  ``cap_points``: polygon points room per page (default
    4 (H + W) + 4096); a page that needs more is redone alone with the room it reported.  Returns, per page, (rescaled polygons [int32 (k, 2)],
    rects int32 [k,5] = (page_ids[p], x, y, w, h), scores float32 [k])."""
    if isinstance(prob_maps, torch.Tensor):
        assert not prob_maps.is_cuda and prob_maps.dtype == torch.float32 and prob_maps.is_contiguous()
        n, H, W = prob_maps.shape[-3:] if prob_maps.dim() >= 3 else (1,) + tuple(prob_maps.shape)
        ptr = prob_maps.data_ptr()
    else:
        prob_maps = np.ascontiguousarray(prob_maps, dtype=np.float32)
        if prob_maps.ndim == 2:
            prob_maps = prob_maps[None]
        n, H, W = prob_maps.shape
        ptr = prob_maps.ctypes.data
    sh = np.ascontiguousarray([s[0] for s in scales], np.float64)
    sw = np.ascontiguousarray([s[1] for s in scales], np.float64)
    oh = np.ascontiguousarray([o[0] for o in orig_sizes], np.int32)
    ow = np.ascontiguousarray([o[1] for o in orig_sizes], np.int32)
    ids = np.ascontiguousarray(np.arange(n) if page_ids is None else page_ids, np.int32)
    assert len(sh) == len(sw) == len(oh) == len(ow) == len(ids) == n
    cap = int(cap_per_page or max(int(post_processor.max_candidates), 1))
    cap_pts = int(4 * (H + W) + 4096 if cap_points is None else cap_points)
    lib = _lib.load()

    def call(i0, i1, cap_pts):
        m = i1 - i0
        pts = np.empty((m, max(cap_pts, 1), 2), np.int32)
        offs = np.empty((m, cap + 1), np.int32)
        rects = np.empty((m, cap, 5), np.int32)
        scores = np.empty((m, cap), np.float32)
        counts, over = np.empty(m, np.int32), np.empty(m, np.int32)
        _lib.check(lib.ocrvi_db_boxes_pages(ptr + i0 * H * W * 4, m, H, W, float(post_processor.thresh), float(post_processor.box_thresh),
                                            int(post_processor.max_candidates), float(post_processor.unclip_ratio), float(post_processor.min_area),
                                            sw[i0:].ctypes.data, sh[i0:].ctypes.data, oh[i0:].ctypes.data, ow[i0:].ctypes.data, ids[i0:].ctypes.data,
                                            pts.ctypes.data, cap_pts, offs.ctypes.data, rects.ctypes.data, scores.ctypes.data, cap,
                                            counts.ctypes.data, over.ctypes.data, int(threads)))
        out = []
        for j in range(m):
            k = int(counts[j])
            if over[j]:
                out.append(None)
                continue
            o = offs[j]
            out.append(([pts[j, o[b]:o[b + 1]].copy() for b in range(k)], rects[j, :k].copy(), scores[j, :k].copy()))
        return out, over

    res, over = call(0, n, cap_pts)
    for j in np.nonzero(over)[0]:          # the page's polygons did not fit: redo it alone with the room it asked for
        res[j] = call(int(j), int(j) + 1, int(over[j]))[0][0]
    return res

class DBComponents:
    """Device half of DB post-processing for a fixed page geometry: ``run(prob)`` thresholds DEVICE maps [n,H,W] and labels their
    8-connected components (``ocrvi_db_components``), leaving in HBM the 1-bit mask, the component table and the probability values
    inside the component boxes; ``to_host()`` (or the enqueue-only ``copy_async()``) copies those -- not the maps -- into one of
    ``host_slots`` pinned buffer sets, and ``boxes()`` finishes the stage on the host (``ocrvi_db_boxes_batch_sparse``), falling back to
    the full map for a page whose table or boxes overflowed.  Replaces the ``.cpu().numpy()`` of the whole map at pipeline2.py:320 plus the
    thresholding at src/det/test.py:57."""

    def __init__(self, n_pages: int, H: int, W: int, device="cuda:0", cap: int = 4096, pack_frac: float = 0.5, host_slots: int = 1):
        assert W % 32 == 0, "page width must be a multiple of 32"
        self.n, self.H, self.W, self.cap = n_pages, H, W, cap
        self.dev = torch.device(device)
        self.devi = _dev_index(self.dev)   # an index-less 'cuda' means the current device, as in DBNetPP / SVTRv2
        self.pack_cap = int(H * W * pack_frac)
        d = dict(device=self.dev)
        self.bits = torch.empty((n_pages, H, W // 32), dtype=torch.int32, **d)
        self.comps = torch.empty((n_pages, cap, 8), dtype=torch.int32, **d)
        self.counts = torch.empty((n_pages,), dtype=torch.int32, **d)
        self.offsets = torch.empty((n_pages, cap + 1), dtype=torch.int64, **d)
        self.packed = torch.empty((n_pages, self.pack_cap), dtype=torch.float32, **d)
        self.ws = torch.empty((_lib.load().ocrvi_db_components_workspace_bytes(n_pages, H, W),), dtype=torch.uint8, **d)
        self._dev_bufs = (self.counts, self.offsets, self.comps, self.bits, self.packed)
        self.host = [tuple(torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._dev_bufs) for _ in range(host_slots)]
        self._select(0)

    def _select(self, slot):
        self.h_counts, self.h_offsets, self.h_comps, self.h_bits, self.h_packed = self.host[slot]

    def run(self, prob: torch.Tensor, thresh: float, n_pages: int = None, stream=None):
        n = n_pages or self.n
        assert prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous() and prob.numel() >= n * self.H * self.W and n <= self.n
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        _lib.check(_lib.load().ocrvi_db_components(self.devi, prob.data_ptr(), n, self.H, self.W, float(thresh), self.bits.data_ptr(),
                                                   self.comps.data_ptr(), self.counts.data_ptr(), self.cap, self.offsets.data_ptr(),
                                                   self.packed.data_ptr(), self.pack_cap, self.ws.data_ptr(), st.cuda_stream))

    def copy_async(self, slot: int = 0, n_pages: int = None, pack_floats: int = None) -> int:
        """Enqueue-only: the tables, the mask and the first ``pack_floats`` (default: all) packed values of every page, on the current
        stream, into host slot ``slot``.  Returns the bytes enqueued.  (A page that packed more than was copied is caught by ``boxes``.)"""
        n = n_pages or self.n
        k = self.pack_cap if pack_floats is None else min(int(pack_floats), self.pack_cap)
        moved = 0
        for h, dv in zip(self.host[slot][:4], self._dev_bufs[:4]):
            h[:n].copy_(dv[:n], non_blocking=True)
            moved += h[:n].numel() * h.element_size()
        self.host[slot][4][:n, :k].copy_(self.packed[:n, :k], non_blocking=True)
        self._copied = k
        return moved + n * k * 4

    def to_host(self, n_pages: int = None, slot: int = 0) -> int:
        """Two-phase copy on the current stream: the small tables first, then only as much of each page's packed values as its table
        says were written.  Returns the bytes that crossed PCIe."""
        n = n_pages or self.n
        self._select(slot)
        moved = 0
        for h, dv in zip(self.host[slot][:4], self._dev_bufs[:4]):
            h[:n].copy_(dv[:n], non_blocking=True)
            moved += h[:n].numel() * h.element_size()
        torch.cuda.current_stream(self.dev).synchronize()
        for pg in range(n):
            c = int(self.h_counts[pg])
            tot = int(self.h_offsets[pg, min(c, self.cap)])
            if 0 < tot <= self.pack_cap and c <= self.cap:
                self.h_packed[pg, :tot].copy_(self.packed[pg, :tot], non_blocking=True)
                moved += tot * 4
        torch.cuda.current_stream(self.dev).synchronize()
        self._copied = self.pack_cap
        return moved

    def boxes(self, post_processor: "DBPostProcessor", prob: torch.Tensor = None, scale_w: float = 1.0, scale_h: float = 1.0,
              orig_hw: Tuple[int, int] = None, page_base: int = 0, threads: int = 8, n_pages: int = None, slot: int = 0, cap_per_page: int = None):
        """Host finish from the buffers of host slot ``slot``.  Returns what ``db_boxes_batch`` returns.  ``prob`` (the device maps) is
        only read for pages that overflowed the table or the packed buffer (or the part of it that was copied)."""
        n = n_pages or self.n
        self._select(slot)
        oh, ow = orig_hw if orig_hw is not None else (self.H, self.W)
        cap = int(cap_per_page or post_processor.max_candidates)
        rects, scores = np.empty((n, cap, 5), np.int32), np.empty((n, cap), np.float32)
        counts, skipped = np.empty(n, np.int32), np.zeros(n, np.int32)
        # pack_cap passed down = what was actually copied: a page with more packed values than that is skipped, not read past the copy
        limit = min(getattr(self, "_copied", self.pack_cap), self.pack_cap)
        lib = _lib.load()
        if limit == self.pack_cap:
            _lib.check(lib.ocrvi_db_boxes_batch_sparse(
                self.h_bits.data_ptr(), self.h_comps.data_ptr(), self.h_counts.data_ptr(), self.cap, self.h_offsets.data_ptr(),
                self.h_packed.data_ptr(), self.pack_cap, n, self.H, self.W, float(post_processor.box_thresh), int(post_processor.max_candidates),
                float(post_processor.unclip_ratio), float(post_processor.min_area), float(scale_w), float(scale_h), int(oh), int(ow), int(page_base),
                rects.ctypes.data, scores.ctypes.data, cap, counts.ctypes.data, int(threads), skipped.ctypes.data))
        else:   # rows of the packed buffer are pack_cap apart but only `limit` floats of each are valid: one page per call
            for pg in range(n):
                _lib.check(lib.ocrvi_db_boxes_batch_sparse(
                    self.h_bits[pg].data_ptr(), self.h_comps[pg].data_ptr(), self.h_counts[pg:].data_ptr(), self.cap, self.h_offsets[pg].data_ptr(),
                    self.h_packed[pg].data_ptr(), limit, 1, self.H, self.W, float(post_processor.box_thresh), int(post_processor.max_candidates),
                    float(post_processor.unclip_ratio), float(post_processor.min_area), float(scale_w), float(scale_h), int(oh), int(ow),
                    int(page_base) + pg, rects[pg].ctypes.data, scores[pg].ctypes.data, cap, counts[pg:].ctypes.data, 1, skipped[pg:].ctypes.data))
        for pg in np.nonzero(skipped)[0]:
            if prob is None:
                raise RuntimeError(f"db components: page {pg} overflowed the component table / packed buffer and no full map was given")
            full = prob.reshape(-1, self.H, self.W)[pg:pg + 1].cpu()
            r, c, sc = db_boxes_batch(full, post_processor, scale_w, scale_h, (oh, ow), page_base + int(pg), 1, cap_per_page=cap)
            counts[pg] = c[0]
            rects[pg, :c[0]] = r
            scores[pg, :c[0]] = sc
        keep = [rects[i, :counts[i]] for i in range(n)]
        return (np.concatenate(keep, 0) if keep else np.empty((0, 5), np.int32)), counts.copy(), \
            np.concatenate([scores[i, :counts[i]] for i in range(n)], 0)


def rescale_boxes(boxes, scale_w: float, scale_h: float) -> List[np.ndarray]:
    """pipeline2.py:324-328: the in-place true-divide into the integer array truncates toward zero; then ``astype(int32)``."""
    out = []
    for box in boxes:
        b = np.asarray(box).astype(np.int64)
        b[:, 0] = np.trunc(b[:, 0] / scale_w)
        b[:, 1] = np.trunc(b[:, 1] / scale_h)
        out.append(b.astype(np.int32))
    return out


def crop_rect(img_hw: Tuple[int, int], box) -> Tuple[int, int, int, int]:
    """The rectangle crop_image (src/det/test.py:123-130) slices: cv2.boundingRect of the integer box, clamped to the image."""
    h, w = img_hw
    pts = np.asarray(box).reshape(-1, 2)
    x0, y0 = int(pts[:, 0].min()), int(pts[:, 1].min())
    bw, bh = int(pts[:, 0].max()) - x0 + 1, int(pts[:, 1].max()) - y0 + 1     # boundingRect of integer points is inclusive
    x, y = max(0, x0), max(0, y0)
    return x, y, max(min(bw, w - x), 0), max(min(bh, h - y), 0)


def crop_image(img: np.ndarray, box) -> np.ndarray:
    x, y, bw, bh = crop_rect(img.shape[:2], box)
    return img[y:y + bh, x:x + bw]


def preprocess_crops(images_u8: torch.Tensor, rects: Sequence[Sequence[int]], img_size: Tuple[int, int] = (32, 256)) -> torch.Tensor:
    """Batched crop + preprocess_for_recognition (pipeline2.py:92-128) on the device.
    images_u8 [N,H,W,3] uint8 on the device; rects = (image index, x, y, w, h) -> float32 [B,3,h,w]."""
    images_u8 = images_u8.contiguous()
    N, H, W, _ = images_u8.shape
    r = torch.as_tensor(np.asarray(rects, dtype=np.int32).reshape(-1, 5), device=images_u8.device)
    out = torch.empty((r.shape[0], 3, img_size[0], img_size[1]), dtype=torch.float32, device=images_u8.device)
    stream = torch.cuda.current_stream(images_u8.device).cuda_stream
    _lib.check(_lib.load().ocrvi_crop_resize_normalize(_dev_index(images_u8.device), images_u8.data_ptr(), N, H, W, r.data_ptr(), r.shape[0],
                                                       img_size[0], img_size[1], out.data_ptr(), stream))
    return out


def _polygons_flat(boxes):
    """A list of (n_i, 2) integer polygons -> (points int32 [total, 2], offsets int32 [n + 1])."""
    polys = [np.asarray(b).reshape(-1, 2) for b in boxes]
    offs = np.zeros(len(polys) + 1, np.int32)
    if polys:
        offs[1:] = np.cumsum([len(p) for p in polys])
    pts = np.concatenate(polys, 0) if polys else np.empty((0, 2), np.int64)
    if pts.size and (pts.min() < -32768 or pts.max() > 32767):
        raise ValueError("min_area_quads: polygon coordinates must lie in [-32768, 32767]")
    return np.ascontiguousarray(pts, np.int32).reshape(-1, 2), offs


def min_area_quads(boxes):
    """The minimum-area rectangle of each polygon of ``boxes`` (``ocrvi_min_area_quads``: exact integer arithmetic, include/ocrvi.h).
    Returns (quads float64 [n, 4, 2], flags int32 [n]); ``flags[i] = 1`` marks a polygon without three hull vertices, whose quad is
    its bounding box.  Needs no GPU."""
    pts, offs = _polygons_flat(boxes)
    n = len(offs) - 1
    quads, flags = np.empty((n, 4, 2), np.float64), np.empty(n, np.int32)
    _lib.check(_lib.load().ocrvi_min_area_quads(pts.ctypes.data, offs.ctypes.data, n, quads.ctypes.data, flags.ctypes.data))
    return quads, flags


def quad_crops(boxes, img_hw: Tuple[int, int], page_id: int = 0):
    """The oriented crop descriptors of the polygons ``boxes`` of an ``img_hw = (h, w)`` page (``ocrvi_min_area_quads`` then
    ``ocrvi_quad_crops``): (crops int32 [n, 4] = (page_id, w, h, 0), m_inv float64 [n, 9]).  A quad the four-point geometry refuses (shorter
    than a pixel, tilted by exactly 45 degrees) and a degenerate polygon fall back to the ``crop_rect`` rectangle under a translation.
    Needs no GPU."""
    quads, flags = min_area_quads(boxes)
    n = len(flags)
    ids = np.full(n, int(page_id), np.int32)
    hw = np.empty((n, 2), np.int32)
    hw[:] = (int(img_hw[0]), int(img_hw[1]))
    crops, m_inv = np.empty((n, 4), np.int32), np.empty((n, 9), np.float64)
    _lib.check(_lib.load().ocrvi_quad_crops(quads.ctypes.data, flags.ctypes.data, n, ids.ctypes.data, hw.ctypes.data, crops.ctypes.data,
                                            m_inv.ctypes.data))
    return crops, m_inv


def preprocess_crops_quad(images_u8: torch.Tensor, crops, m_inv, img_size: Tuple[int, int] = (32, 256)) -> torch.Tensor:
    """``preprocess_crops`` for oriented crops (``ocrvi_crop_quad_resize_normalize``): images_u8 [N,H,W,3] uint8 on the device; crops
    int32 [B, 4] = (image index, w, h, 0) and m_inv float64 [B, 9] as ``quad_crops`` returns them -> float32 [B,3,h,w]."""
    images_u8 = images_u8.contiguous()
    N, H, W, _ = images_u8.shape
    c = torch.as_tensor(np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 4)), device=images_u8.device)
    m = torch.as_tensor(np.ascontiguousarray(np.asarray(m_inv, dtype=np.float64).reshape(-1, 9)), device=images_u8.device)
    if m.shape[0] != c.shape[0]:
        raise ValueError(f"preprocess_crops_quad: {c.shape[0]} crops but {m.shape[0]} matrices")
    out = torch.empty((c.shape[0], 3, img_size[0], img_size[1]), dtype=torch.float32, device=images_u8.device)
    stream = torch.cuda.current_stream(images_u8.device).cuda_stream
    _lib.check(_lib.load().ocrvi_crop_quad_resize_normalize(_dev_index(images_u8.device), images_u8.data_ptr(), N, H, W, c.data_ptr(), m.data_ptr(),
                                                            c.shape[0], img_size[0], img_size[1], out.data_ptr(), stream))
    return out


CROP_MODES = ("rect", "quad")


def _check_crop(crop) -> str:
    if crop not in CROP_MODES:
        raise ValueError(f"crop: expected 'rect' or 'quad', got {crop!r}")
    return crop


def preprocess_for_recognition(crop: np.ndarray, img_size: Tuple[int, int] = (32, 256), device: str = "cuda:0") -> torch.Tensor:
    """pipeline2.py:92-128 for one crop (HxWx3 uint8, or HxW grey which is replicated as cv2.COLOR_GRAY2RGB does) -> [3,h,w]."""
    if crop.ndim == 2:
        crop = np.repeat(crop[:, :, None], 3, axis=2)
    crop = np.ascontiguousarray(crop[:, :, :3])
    if crop.size == 0:
        return torch.zeros((3,) + tuple(img_size), device=device)
    img = torch.from_numpy(crop).to(device)[None]
    return preprocess_crops(img, [(0, 0, 0, crop.shape[1], crop.shape[0])], img_size)[0]


def recognize_text(model: SVTRv2, crop: np.ndarray, device: str = "cuda:0", img_size: Tuple[int, int] = (32, 256)) -> str:
    """pipeline2.py:131-141."""
    out = recognize_text_batch(model, [crop], device, img_size, 1)
    return out[0] if out else ""


def recognize_text_batch(model: SVTRv2, crops: List[np.ndarray], device: str = "cuda:0", img_size: Tuple[int, int] = (32, 256),
                         batch_size: int = 32, return_confidence: bool = False, beam: Optional[int] = None, nbest: int = 1,
                         lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
    """pipeline2.py:144-168: batches of ``batch_size`` crops -> forward -> greedy CTC strings.  Empty crops become the all-zero tensor
    of :154-156.  ``return_confidence=True``: a list of ``rec.Recognition`` instead, whose ``text`` are those strings.
    ``beam=W``: one list of ``rec.Hypothesis`` per crop instead (``SVTRv2.decode_greedy(..., beam=W, nbest=nbest)``: best first, at most
    ``nbest``); ValueError together with ``return_confidence=True``.  ``lm=CharLM`` (with ``beam``; ``lm_weight``, ``len_bonus``): the search
    with the language model fused in, lists of ``rec.LMHypothesis``; ValueError as ``SVTRv2.decode_probs`` raises it."""
    check_beam(beam, nbest, img_size[1] // 4, return_confidence)
    check_lm(lm, lm_weight, len_bonus, beam, model.tokenizer.num_classes, model.blank_id)
    texts = []
    for i in range(0, len(crops), batch_size):
        ts = [preprocess_for_recognition(c, img_size, device) for c in crops[i:i + batch_size]]
        if beam is not None:
            texts.extend(model.decode_greedy(torch.stack(ts), beam=beam, nbest=nbest, lm=lm, lm_weight=lm_weight, len_bonus=len_bonus))
            continue
        texts.extend(model.decode_greedy(torch.stack(ts), True) if return_confidence else model.decode_greedy(torch.stack(ts)))
    return texts


def char_boxes(rect, rec: Recognition, rec_size: Tuple[int, int] = (32, 256)) -> np.ndarray:
    """Where the characters of a recognised rectangle crop sit on the page: ``rect = (x, y, w, h)`` as ``crop_rect`` gives it, ``rec`` the
    crop's ``Recognition`` -> int32 [len(rec.text), 4] rectangles (x, y, w, h).  Step t of the recogniser stands for columns [4t, 4t + 4) of
    the resized crop, clipped to its resized width ``rw`` (the ``new_w`` of ``preprocess_for_recognition``: ``int(w * (rec_h / h))``, at
    most ``rec_size[1]``, at least 1); a span (t0, t1) covers resized columns [c0, c1) = [4 t0, 4 t1 + 4) and maps back in integers:
    ``x0 = x + (c0 * w) // rw``, ``x1 = x + ceil(c1 * w / rw)`` clipped to ``x + w``, the width at least 1 and inside the crop (a span that
    lies in the padding right of ``rw`` gives the crop's last column).  ``y`` and ``h`` are the crop's.
    Greedy CTC spans are peaky -- the network commits to a character on a step or two and emits blank around it -- so these boxes are
    approximate: they say where the character was decided, not its full extent.  Oriented (quad) crops are not supported: ValueError."""
    r = np.asarray(rect)
    if r.shape != (4,) or r.dtype.kind not in "iu":
        raise ValueError(f"char_boxes: expected an integer rectangle (x, y, w, h), got shape {r.shape} dtype {r.dtype} "
                         "(oriented crops are not supported)")
    x, y, w, h = (int(v) for v in r)
    if w <= 0 or h <= 0:
        raise ValueError(f"char_boxes: empty rectangle {w}x{h}")
    rw = max(min(int(w * (rec_size[0] / h)), int(rec_size[1])), 1)
    out = np.empty((len(rec.spans), 4), np.int32)
    for i, (t0, t1) in enumerate(rec.spans):
        c0, c1 = min(4 * t0, rw), min(4 * t1 + 4, rw)
        x0 = min(x + (c0 * w) // rw, x + w - 1)
        x1 = min(x + -((-c1 * w) // rw), x + w)
        out[i] = (x0, y, max(x1 - x0, 1), h)
    return out


def as_quad(pts, what: str = "quad") -> np.ndarray:
    """The four corners as a float64 [4, 2] array; ValueError (starting with ``what``) for another shape or a non-finite value.  (4, 1, 2), the
    layout of a cv2 contour, is accepted as ``screen_cnt.reshape(4, 2)`` accepts it (scanner.py:187)."""
    try:
        q = np.asarray(pts, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected four (x, y) corners, got {type(pts).__name__}") from None
    if q.shape == (4, 1, 2):
        q = q.reshape(4, 2)
    if q.shape != (4, 2):
        raise ValueError(f"{what}: expected four (x, y) corners (shape (4, 2)), got shape {q.shape}")
    if not np.isfinite(q).all():
        raise ValueError(f"{what}: a corner is not finite")
    return np.ascontiguousarray(q)


def four_point_geometry(pts, what: str = "quad"):
    """The host half of four_point_transform (scanner.py:33-50, ``ocrvi_four_point_transform``): corner order, output size and the two
    matrices.  Returns (m_fwd float64 [3,3] source -> rectified, m_inv float64 [3,3], out_w, out_h).  Needs no GPU.  ValueError when the
    quad rectifies to less than one pixel or its ordered corners are degenerate (the reference passes those to cv2)."""
    q = as_quad(pts, what)
    m_fwd, m_inv = np.empty(9, np.float64), np.empty(9, np.float64)
    w, h = ctypes.c_int32(0), ctypes.c_int32(0)
    lib = _lib.load()
    rc = lib.ocrvi_four_point_transform(q.ctypes.data, m_fwd.ctypes.data, m_inv.ctypes.data, ctypes.byref(w), ctypes.byref(h))
    if rc == -1:
        raise ValueError(f"{what}: {_lib.last_error()}")
    _lib.check(rc)
    return m_fwd.reshape(3, 3), m_inv.reshape(3, 3), w.value, h.value


def warp_perspective(image: torch.Tensor, m_inv, out_h: int, out_w: int) -> torch.Tensor:
    """``ocrvi_warp_perspective_u8`` on the current stream: uint8 HxWx3 device tensor -> uint8 out_h x out_w x 3 device tensor under the
    destination -> source matrix ``m_inv`` (cv2.warpPerspective(image, M, (out_w, out_h)) with m_inv = M^-1, scanner.py:51)."""
    assert image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
    image = image.contiguous()
    m = np.ascontiguousarray(np.asarray(m_inv, np.float64).reshape(9))
    out = torch.empty((int(out_h), int(out_w), 3), dtype=torch.uint8, device=image.device)
    stream = torch.cuda.current_stream(image.device).cuda_stream
    _lib.check(_lib.load().ocrvi_warp_perspective_u8(_dev_index(image.device), image.data_ptr(), image.shape[0], image.shape[1], m.ctypes.data,
                                                     out.data_ptr(), int(out_h), int(out_w), stream))
    return out


def four_point_transform(image, pts, device: str = "cuda:0"):
    """scanner.py:29-53: the document whose corners are ``pts`` (four (x, y) points of ``image``, any order) flattened to a
    max_width x max_height page.  The geometry runs on the host, the warp on the device.  ``image``: uint8 HxWx3, a numpy array (the
    result is a numpy array) or a device tensor (the result stays on its device)."""
    _, m_inv, w, h = four_point_geometry(pts)
    if isinstance(image, torch.Tensor) and image.is_cuda:
        return warp_perspective(image, m_inv, h, w)
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"four_point_transform: expected a uint8 HxWx3 image, got dtype {img.dtype} shape {tuple(img.shape)}")
    out = warp_perspective(img.to(device), m_inv, h, w).cpu()
    return out if isinstance(image, torch.Tensor) else out.numpy()


_ENHANCE_READY = set()


def enhance_init(devi: int) -> None:
    """``ocrvi_enhance_init`` once per device index (it allocates and synchronises: never inside a capture)."""
    if devi not in _ENHANCE_READY:
        _lib.check(_lib.load().ocrvi_enhance_init(devi))
        _ENHANCE_READY.add(devi)


def enhance_workspace_bytes(h: int, w: int) -> int:
    n = ctypes.c_size_t()
    rc = _lib.load().ocrvi_enhance_workspace_bytes(int(h), int(w), ctypes.byref(n))
    if rc == -1:
        raise ValueError(f"enhance_document: {_lib.last_error()}")
    _lib.check(rc)
    return n.value


def enhance_page(image: torch.Tensor) -> torch.Tensor:
    """``ocrvi_enhance_u8`` on the current stream: uint8 HxWx3 RGB device tensor -> the enhanced page, a new tensor on the same device."""
    assert image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
    image = image.contiguous()
    h, w = int(image.shape[0]), int(image.shape[1])
    devi = _dev_index(image.device)
    ws = torch.empty(enhance_workspace_bytes(h, w), dtype=torch.uint8, device=image.device)
    enhance_init(devi)
    out = torch.empty_like(image)
    stream = torch.cuda.current_stream(image.device).cuda_stream
    _lib.check(_lib.load().ocrvi_enhance_u8(devi, image.data_ptr(), h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return out


def enhance_document(image, device: str = "cuda:0"):
    """scanner.py:55-76, the reference's "Magic Color": Lab -> CLAHE(2.0, 8 x 8) on L -> RGB -> non-local-means denoising (10, 10, 7, 21)
    -> 3 x 3 sharpening, all on the device (``ocrvi_enhance_u8``; the arithmetic is stated in include/ocrvi.h, parity with cv2 is
    unpinned).  ``image``: RGB uint8 HxWx3 with both sides >= 16, a numpy array (the result is a numpy array) or a device tensor (the
    result stays on its device).  ValueError for a smaller page."""
    if isinstance(image, torch.Tensor) and image.is_cuda:
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError(f"enhance_document: expected a uint8 HxWx3 image, got dtype {image.dtype} shape {tuple(image.shape)}")
        return enhance_page(image)
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"enhance_document: expected a uint8 HxWx3 image, got dtype {img.dtype} shape {tuple(img.shape)}")
    enhance_workspace_bytes(img.shape[0], img.shape[1])       # the size check, before anything is uploaded
    out = enhance_page(img.to(device)).cpu()
    return out if isinstance(image, torch.Tensor) else out.numpy()


def preprocess_image(image, quad, enhance: bool = False, device: str = "cuda:0"):
    """scanner.py:168-196 with the document's corners supplied by the caller instead of found by the rembg network (``quad`` is what
    ``screen_cnt.reshape(4, 2) * ratio`` is there, :187).  ``quad=None`` returns the image, as the reference does when no document is
    found (:183-184).  ``enhance=True`` still raises here (the pipeline calls this stage with enhance=False, pipeline2.py:296): the
    enhancement is its own call, ``enhance_document(preprocess_image(image, quad))``, or ``enhance=True`` of ``detect_and_recognize``."""
    if enhance:
        raise NotImplementedError("preprocess_image(enhance=True): call pipeline.enhance_document(preprocess_image(image, quad)) instead "
                                  "(enhance_document, scanner.py:55-76: CLAHE, non-local-means denoising, sharpening, runs on the device "
                                  "as a stage of its own)")
    if quad is None:
        return image
    return four_point_transform(image, quad, device)


# ---------------------------------------------------------------------------------------------------- document finder
DOC_KINDS = (None, "polygon", "rectangle")        # ocrvi_document_contour's `found`


def find_document_contour(mask, return_kind: bool = False):
    """scanner.py:104-132, the half of ``find_document_contour_dl`` after its network (``ocrvi_document_contour``, host only, needs no GPU):
    ``mask`` is any 2-D uint8 / bool segmentation (non-zero = document; rembg's alpha channel is one) -> the reference's ``screen_cnt`` as
    an int32 [4, 2] array of (x, y) in mask coordinates, or ``None`` when the mask is empty.  External contours, the five largest by area, the
    first whose ``approxPolyDP(0.02 * arcLength)`` has four points, else the minimum-area rectangle of the largest.  ``return_kind=True``
    returns (quad, "polygon" / "rectangle" / None).  The definition is in include/ocrvi.h; parity with cv2 is unpinned."""
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.view(np.uint8)
    if m.dtype != np.uint8 or m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"find_document_contour: expected a 2-D uint8 mask, got dtype {m.dtype} shape {m.shape}")
    if m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(m)
    quad, found = np.zeros((4, 2), np.int32), ctypes.c_int32(0)
    rc = _lib.load().ocrvi_document_contour(m.ctypes.data, m.shape[0], m.shape[1], m.strides[0], quad.ctypes.data, ctypes.byref(found))
    if rc == -1:
        raise ValueError(f"find_document_contour: {_lib.last_error()}")
    _lib.check(rc)
    q = quad if found.value else None
    return (q, DOC_KINDS[found.value]) if return_kind else q


def doc_working_size(h: int, w: int, work_h: int = _lib.DOC_WORK_H) -> Tuple[int, float]:
    """``ocrvi_doc_working_size``: (ww, ratio) of an h x w page at ``work_h`` working rows (scanner.py:85-86); ValueError outside the bounds
    the header states (8 <= ww <= 8192, sides <= 16384, 8 <= work_h <= 512)."""
    ww, ratio = ctypes.c_int32(0), ctypes.c_double(0)
    rc = _lib.load().ocrvi_doc_working_size(int(h), int(w), int(work_h), ctypes.byref(ww), ctypes.byref(ratio))
    if rc == -1:
        raise ValueError(f"document finder: {_lib.last_error()}")
    _lib.check(rc)
    return ww.value, ratio.value


def _doc_polarity(polarity) -> int:
    try:
        return _lib.DOC_POLARITIES[polarity]
    except (KeyError, TypeError):
        raise ValueError(f"polarity: expected one of {sorted(_lib.DOC_POLARITIES)}, got {polarity!r}") from None


def doc_mask_bits(pages: Sequence[torch.Tensor], work_h: int = _lib.DOC_WORK_H, polarity="auto"):
    """``ocrvi_doc_mask_pages`` on the current stream for device pages (uint8 HxWx3, one device) of any sizes: one page table, one launch
    per stage.  Returns (bits, sizes): ``bits`` an int32 device tensor [n, work_h * ((ww_cap + 31) // 32)] whose row i holds page i's mask
    in the layout of ITS OWN ww (bit x & 31 of word y * ((ww + 31) // 32) + (x >> 5)), ``sizes`` a list of (ww, ratio), ``None`` for a page
    outside the bounds of ``doc_working_size`` (its row is all zero)."""
    pol = _doc_polarity(polarity)
    pages = [p.contiguous() for p in pages]
    sizes = []
    for p in pages:
        try:
            sizes.append(doc_working_size(p.shape[0], p.shape[1], work_h))
        except ValueError:
            sizes.append(None)
    lib, device, n = _lib.load(), pages[0].device, len(pages)
    ww_cap = max([s[0] for s in sizes if s is not None] + [8])
    ws_bytes, words = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(lib.ocrvi_doc_mask_sizes(n, int(work_h), ww_cap, ctypes.byref(ws_bytes), ctypes.byref(words)))
    with torch.cuda.device(device):
        table = torch.tensor([(p.data_ptr(), p.shape[0], p.shape[1], 0) for p in pages], dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=device)
        bits = torch.empty((n, words.value), dtype=torch.int32, device=device)
        _lib.check(lib.ocrvi_doc_mask_pages(_dev_index(device), table.data_ptr(), n, int(work_h), ww_cap, pol, bits.data_ptr(), ws.data_ptr(),
                                            ws.numel(), torch.cuda.current_stream(device).cuda_stream))
    return bits, sizes                            # (table and workspace go back to the allocator of the stream the launches are on)


def _check_rgb(image, what: str):
    if not isinstance(image, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{what}: expected an RGB uint8 HxWx3 numpy array or tensor, got {type(image).__name__}")
    if image.dtype != (np.uint8 if isinstance(image, np.ndarray) else torch.uint8) or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"{what}: expected a uint8 HxWx3 image, got dtype {image.dtype} shape {tuple(image.shape)}")


def document_mask(image, work_h: int = _lib.DOC_WORK_H, polarity="auto", device: str = "cuda:0"):
    """The library's own document mask (include/ocrvi.h, "Document finder", part B): area-average luminance at ``work_h`` rows (500, the
    reference's working height, scanner.py:85-86) -> binomial smooth -> Otsu -> polarity (``"auto"``: the frame is background; ``"bright"``
    / ``"dark"``: the document is) -> 5 x 5 opening, all on the device.  Returns (mask uint8 [work_h, ww] of 0 / 255, ratio): a numpy array
    for a host image, a device tensor for a device tensor.  It tells a document from its background by brightness alone; feed the mask to
    ``find_document_contour``.  ValueError for a page outside the bounds of ``doc_working_size``."""
    _check_rgb(image, "document_mask")
    on_device = isinstance(image, torch.Tensor) and image.is_cuda
    ww, ratio = doc_working_size(image.shape[0], image.shape[1], work_h)
    img = image if on_device else torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray) else image).to(device)
    bits, _ = doc_mask_bits([img], work_h, polarity)
    wpr = (ww + 31) // 32
    b = bits[0, :work_h * wpr].view(work_h, wpr, 1) >> torch.arange(32, dtype=torch.int32, device=bits.device)
    mask = ((b & 1).to(torch.uint8) * 255).view(work_h, wpr * 32)[:, :ww].contiguous()
    if on_device:
        return mask, ratio
    mask = mask.cpu()
    return (mask.numpy() if isinstance(image, np.ndarray) else mask), ratio


def find_document_quads(images, polarity="auto", device: str = "cuda:0"):
    """``find_document_contour_dl`` (scanner.py:78-132) with the library's own mask in the network's place, for a list of pages of any
    sizes: host arrays, device tensors, JPEG bytes or PNG bytes.  Encoded pages are decoded in one batch per format, host pages are
    uploaded, all pages go through one page table and one launch per stage (``ocrvi_doc_mask_pages``); only the bit masks, about 23 KB
    a page, come back, and the host traces them (``ocrvi_document_contour_bits``).  Returns per page the corners as float64 [4, 2] in the
    page's coordinates -- the contour scaled by the ratio, ``screen_cnt.reshape(4, 2) * ratio`` (scanner.py:187), what ``preprocess_image``
    and ``Engine.run`` take as ``quad`` -- or ``None`` when nothing is found (an empty or constant page, a page outside the bounds of
    ``doc_working_size``).  The quad is returned as found: a degenerate one is refused by ``four_point_geometry`` as before."""
    images = list(images)
    if not images:
        return []
    dev = torch.device(device)
    enc = [i for i, p in enumerate(images) if isinstance(p, IMAGE_BYTES)]
    pages = list(images)
    for i, page in zip(enc, imdecode([images[i] for i in enc], dev) if enc else []):
        pages[i] = page
    for i, p in enumerate(pages):
        _check_rgb(p, f"find_document_quads: page {i}")
        if not (isinstance(p, torch.Tensor) and p.is_cuda):
            pages[i] = torch.as_tensor(np.ascontiguousarray(p) if isinstance(p, np.ndarray) else p).to(dev)
    work_h = _lib.DOC_WORK_H
    bits, sizes = doc_mask_bits(pages, work_h, polarity)
    host = bits.cpu().numpy()
    lib = _lib.load()

    def finish(i):                                # the host half of page i: ctypes drops the interpreter lock, pages trace in parallel
        if sizes[i] is None:
            return None
        quad, found = np.zeros((4, 2), np.int32), ctypes.c_int32(0)
        _lib.check(lib.ocrvi_document_contour_bits(host[i].ctypes.data, work_h, sizes[i][0], quad.ctypes.data, ctypes.byref(found)))
        return quad.astype(np.float64) * sizes[i][1] if found.value else None

    if len(pages) > 1:
        return list(host_pool().map(finish, range(len(pages))))
    return [finish(0)]


def find_document_quad(image, polarity="auto", device: str = "cuda:0"):
    """``find_document_quads`` for one page: float64 [4, 2] or ``None``.  ``preprocess_image(image, find_document_quad(image))`` is the
    reference's ``preprocess_image`` (scanner.py:168-196) with the library's mask in the network's place."""
    return find_document_quads([image], polarity, device)[0]


# ---------------------------------------------------------------------------------------------------- skew estimate
class Skew(NamedTuple):
    """``ocrvi_skew_pick``: the slope index ``k`` (-128 .. 128; the text lines' image slope is k / 512, y pointing down), ``angle`` =
    atan(k / 512) in degrees, and ``gain`` = S_k / S_0, how much sharper the projection profile is along that slope than along the rows."""
    k: int
    angle: float
    gain: float


def skew_scores(pages: Sequence[torch.Tensor], work_h: int = _lib.DOC_WORK_H):
    """``ocrvi_skew_scores_pages`` on the current stream for device pages (uint8 HxWx3, one device) of any sizes: one page table, one launch
    per stage (grey, edges, scores).  Returns (scores, valid): an int64 device tensor [n, 257] holding the uint64 scores S_k at column
    k + 128, and per page whether it lies inside the bounds of ``doc_working_size`` (otherwise its row is zero)."""
    pages = [p.contiguous() for p in pages]
    wws = []
    for p in pages:
        try:
            wws.append(doc_working_size(p.shape[0], p.shape[1], work_h)[0])
        except ValueError:
            wws.append(None)
    lib, device, n = _lib.load(), pages[0].device, len(pages)
    ww_cap = max([w for w in wws if w is not None] + [8])
    ws_bytes = ctypes.c_size_t(0)
    _lib.check(lib.ocrvi_skew_sizes(n, int(work_h), ww_cap, ctypes.byref(ws_bytes)))
    with torch.cuda.device(device):
        table = torch.tensor([(p.data_ptr(), p.shape[0], p.shape[1], 0) for p in pages], dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=device)
        scores = torch.empty((n, _lib.SKEW_ANGLES), dtype=torch.int64, device=device)
        _lib.check(lib.ocrvi_skew_scores_pages(_dev_index(device), table.data_ptr(), n, int(work_h), ww_cap, scores.data_ptr(), ws.data_ptr(),
                                               ws.numel(), torch.cuda.current_stream(device).cuda_stream))
    return scores, [w is not None for w in wws]


def skew_pick(scores) -> Skew:
    """``ocrvi_skew_pick`` (host only): 257 uint64 scores -> ``Skew``."""
    s = np.ascontiguousarray(np.asarray(scores).reshape(_lib.SKEW_ANGLES)).view(np.uint64)
    k, angle, gain = ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.load().ocrvi_skew_pick(s.ctypes.data, ctypes.byref(k), ctypes.byref(angle), ctypes.byref(gain)))
    return Skew(k.value, angle.value, gain.value)


def skew_quad(h: int, w: int, k: int) -> np.ndarray:
    """``ocrvi_skew_quad`` (host only): the corners, float64 [4, 2] of (x, y), of the upright rectangle in the frame turned by slope index
    ``k`` that encloses the whole h x w page -- what ``four_point_transform`` / ``Engine.run`` take to straighten the page; nothing of the page
    is lost, the wedges outside it come out 0.  ``k = 0`` gives the page's own corners."""
    quad = np.zeros((4, 2), np.float64)
    _lib.check(_lib.load().ocrvi_skew_quad(int(h), int(w), int(k), quad.ctypes.data))
    return quad


def estimate_skews(images, work_h: int = _lib.DOC_WORK_H, device: str = "cuda:0"):
    """By how much each page is rotated (include/ocrvi.h, "Skew estimate"), for a list of pages of any sizes: host arrays, device tensors,
    JPEG bytes or PNG bytes, as ``find_document_quads`` takes them.  All pages go through one page table and one launch per stage
    (``ocrvi_skew_scores_pages``); 2 KB of scores per page come back and the host picks (``ocrvi_skew_pick``).  Returns one ``Skew`` per
    page, ``None`` for a page outside the bounds of ``doc_working_size``.  The range is +-14 degrees in steps of 0.11; a turn of 90 or 180
    degrees is not seen."""
    images = list(images)
    if not images:
        return []
    dev = torch.device(device)
    enc = [i for i, p in enumerate(images) if isinstance(p, IMAGE_BYTES)]
    pages = list(images)
    for i, page in zip(enc, imdecode([images[i] for i in enc], dev) if enc else []):
        pages[i] = page
    for i, p in enumerate(pages):
        _check_rgb(p, f"estimate_skews: page {i}")
        if not (isinstance(p, torch.Tensor) and p.is_cuda):
            pages[i] = torch.as_tensor(np.ascontiguousarray(p) if isinstance(p, np.ndarray) else p).to(dev)
    scores, valid = skew_scores(pages, work_h)
    host = scores.cpu().numpy()
    return [skew_pick(host[i]) if ok else None for i, ok in enumerate(valid)]


def estimate_skew(image, work_h: int = _lib.DOC_WORK_H, device: str = "cuda:0"):
    """``estimate_skews`` for one page: a ``Skew`` or ``None``."""
    return estimate_skews([image], work_h, device)[0]


def deskew(image, min_gain: float = 1.0, device: str = "cuda:0"):
    """-> (image, Skew): the page straightened by ``four_point_transform(image, skew_quad(h, w, k))`` when the estimate has ``k != 0`` and
    ``gain >= min_gain``; otherwise -- and for a page outside the bounds, whose Skew is ``None`` -- the image comes back untouched.  The
    straightened page is larger than the original: it encloses all of it."""
    if isinstance(image, IMAGE_BYTES):
        image = imdecode(image, device)
    skew = estimate_skew(image, device=image.device if isinstance(image, torch.Tensor) and image.is_cuda else device)
    if skew is None or skew.k == 0 or not skew.gain >= min_gain:
        return image, skew
    return four_point_transform(image, skew_quad(image.shape[0], image.shape[1], skew.k), device), skew


# ---------------------------------------------------------------------------------------------------- result overlay
def _overlay_rgb(c, what: str) -> int:
    try:
        r, g, b = (int(v) for v in c)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected three integers 0..255, got {c!r}") from None
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"{what}: expected three integers 0..255, got {c!r}")
    return r | g << 8 | b << 16


def _overlay_vertices(polys, names) -> np.ndarray:
    """``box.astype(np.int32)`` (pipeline2.py:176) for every box at once, the range checked first: int32 [total, 2].  ``polys``: the
    boxes as arrays of shape (n_i, 2) (empty ones of any shape); ``names(j)`` describes box j in an error message."""
    for j, v in enumerate(polys):
        if v.size and (v.dtype.kind not in "iuf" or v.ndim != 2 or v.shape[1] != 2):
            raise ValueError(f"{names(j)}: expected an (n, 2) array of numbers, got dtype {v.dtype} shape {v.shape}")
    full = [v for v in polys if v.size]
    if not full:
        return np.empty((0, 2), np.int32)
    pts = np.concatenate(full, 0)
    if pts.dtype.kind == "f":
        pts = np.trunc(pts)
    ok = np.abs(pts) <= _lib.OVERLAY_MAX_COORD          # (False for NaN)
    if not ok.all():
        row = int(np.argmin(ok.all(1)))
        j = int(np.searchsorted(np.cumsum([len(v) if v.size else 0 for v in polys]), row, side="right"))
        raise ValueError(f"{names(j)}: vertices must lie in [-{_lib.OVERLAY_MAX_COORD}, {_lib.OVERLAY_MAX_COORD}]")
    return np.ascontiguousarray(pts, np.int32)


def overlay_segments(boxes_per_page, texts_per_page, sizes, color=(0, 255, 0), label_color=(255, 0, 0), thickness: int = 2):
    """``ocrvi_overlay_segments`` (host only, needs no GPU): the segments and primitives ``draw_boxes_pages`` paints for pages of
    ``sizes[p] = (h, w)``: (segs int32 [n, 8], prims int32 [m, 8], prim_offs int32 [pages + 1]); include/ocrvi.h states the fields, the
    painting rule, the segment order and the digit strokes.  ``texts_per_page`` is None or, per page, None or the page's texts: only
    ``min(len(boxes), len(texts))`` pairs are drawn, as the reference's zip does.  ValueError for what the entry refuses."""
    n = len(boxes_per_page)
    if len(sizes) != n or (texts_per_page is not None and len(texts_per_page) != n):
        raise ValueError(f"overlay: {n} box lists, {len(sizes)} pages, {None if texts_per_page is None else len(texts_per_page)} text lists")
    if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)):
        raise ValueError(f"overlay: thickness {thickness!r} (an integer 1..15 expected)")
    box_rgb, label_rgb = _overlay_rgb(color, "overlay: color"), _overlay_rgb(label_color, "overlay: label_color")
    polys, page_boxes, pairs = [], [0], []
    none = np.empty((0, 2), np.int32)
    for p, boxes in enumerate(boxes_per_page):
        texts = None if texts_per_page is None else texts_per_page[p]
        pairs.append(len(boxes) if texts is None else min(len(boxes), len(texts)))
        # a box past the last pair is never drawn and, as under the reference's zip, never looked at: it travels as a box without vertices
        polys.extend(np.asarray(b) if j < pairs[-1] else none for j, b in enumerate(boxes))
        page_boxes.append(len(polys))

    def names(j):
        p = int(np.searchsorted(page_boxes, j, side="right")) - 1
        return f"overlay: page {p} box {j - page_boxes[p]}"

    pts = _overlay_vertices(polys, names)
    offs = np.zeros(len(polys) + 1, np.int32)
    if polys:
        offs[1:] = np.cumsum([len(v) if v.size else 0 for v in polys])
    page_boxes, pairs = np.asarray(page_boxes, np.int32), np.asarray(pairs, np.int32)
    hw = np.ascontiguousarray(np.asarray([(int(h), int(w)) for h, w in sizes], np.int64).reshape(n, 2).clip(-1, 1 << 30), np.int32)
    lib = _lib.load()
    ns, npr = ctypes.c_int64(), ctypes.c_int64()

    # the documented upper bound sizes the tables: sum n_i + 7 digits segments, two primitives per pair (one call, which validates everything)
    total = int(pairs.sum())
    segs = np.empty((len(pts) + 7 * len(str(max(int(pairs.max()) if n else 0, 1))) * total, _lib.OVERLAY_SEG), np.int32)
    prims, prim_offs = np.empty((2 * total, _lib.OVERLAY_PRIM), np.int32), np.zeros(n + 1, np.int32)
    _lib.check(lib.ocrvi_overlay_segments(pts.ctypes.data, offs.ctypes.data, page_boxes.ctypes.data, pairs.ctypes.data, hw.ctypes.data, n, box_rgb,
                                          label_rgb, int(thickness), segs.ctypes.data, len(segs), prims.ctypes.data, len(prims),
                                          prim_offs.ctypes.data, ctypes.byref(ns), ctypes.byref(npr)))
    return segs[:ns.value], prims[:npr.value], prim_offs


def overlay_upload(pages: Sequence[torch.Tensor], segs: np.ndarray, prims: np.ndarray, prim_offs: np.ndarray) -> Tuple[torch.Tensor, tuple]:
    """The page table of the device pages ``pages`` and the three tables of ``overlay_segments`` in one pinned buffer and one copy:
    (the device buffer, the arguments of ``ocrvi_overlay_pages`` after the device index).  Every table starts on a 16-byte boundary."""
    n = len(pages)
    o_offs = n * _lib.PAGE_ENTRY * 2            # in int32 words
    o_prims = o_offs + (n + 1 + 3) // 4 * 4
    o_segs = o_prims + prims.size
    host = torch.zeros(o_segs + max(segs.size, 4), dtype=torch.int32).pin_memory()
    h = host.numpy()
    h[:o_offs].view(np.int64).reshape(n, _lib.PAGE_ENTRY)[:] = [(t.data_ptr(), t.shape[0], t.shape[1], 0) for t in pages]
    h[o_offs:o_offs + n + 1] = prim_offs
    h[o_prims:o_segs] = prims.reshape(-1)
    h[o_segs:o_segs + segs.size] = segs.reshape(-1)
    dev = host.to(pages[0].device, non_blocking=True)
    base = dev.data_ptr()
    return dev, (base, n, base + 4 * o_prims, base + 4 * o_segs, base + 4 * o_offs, max(t.shape[0] for t in pages), max(t.shape[1] for t in pages))


def overlay_paint_(pages: Sequence[torch.Tensor], segs: np.ndarray, prims: np.ndarray, prim_offs: np.ndarray) -> None:
    """Paints the contiguous device pages ``pages`` IN PLACE on the current stream: one upload, one ``ocrvi_overlay_pages`` launch."""
    if not len(pages) or not len(prims):
        return                                  # nothing to paint
    device = pages[0].device
    with torch.cuda.device(device):
        dev, args = overlay_upload(pages, segs, prims, prim_offs)
        _lib.check(_lib.load().ocrvi_overlay_pages(_dev_index(device), *args, torch.cuda.current_stream(device).cuda_stream))


def draw_boxes_pages(images, boxes_per_page, texts_per_page=None, color=(0, 255, 0), label_color=(255, 0, 0), thickness: int = 2,
                     device: str = "cuda:0") -> List[torch.Tensor]:
    """``draw_boxes_with_text`` for a list of pages of any sizes: one segment build on the host (``ocrvi_overlay_segments``), one upload
    of the tables and one launch (``ocrvi_overlay_pages``) serve all pages.  Returns a list of new device tensors; no input is written."""
    images = list(images)
    sizes = []
    for i, im in enumerate(images):
        if not isinstance(im, (np.ndarray, torch.Tensor)):
            raise ValueError(f"draw_boxes: page {i}: expected a numpy array or a tensor, got {type(im).__name__}")
        if im.dtype not in (np.uint8, torch.uint8) or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"draw_boxes: page {i}: expected an RGB uint8 HxWx3 page, got dtype {im.dtype} shape {tuple(im.shape)}")
        sizes.append((int(im.shape[0]), int(im.shape[1])))
    if len(boxes_per_page) != len(images):
        raise ValueError(f"draw_boxes: {len(boxes_per_page)} box lists for {len(images)} pages")
    if not images:
        return []
    tables = overlay_segments(boxes_per_page, texts_per_page, sizes, color, label_color, thickness)   # (every ValueError before device work)
    dev = torch.device(device)
    outs = []
    for im in images:                           # the reference's .copy() (pipeline2.py:174): always a new tensor
        src = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
        out = torch.empty(tuple(src.shape), dtype=torch.uint8, device=dev)
        out.copy_(src)
        outs.append(out)
    overlay_paint_(outs, *tables)
    return outs


def draw_boxes_with_text(image, boxes, texts=None, color=(0, 255, 0), label_color=(255, 0, 0), thickness: int = 2,
                         device: str = "cuda:0") -> torch.Tensor:
    """``draw_boxes_with_text(image, boxes, texts)`` of the reference (pipeline2.py:173-190, called at :358-360) on the device: every box
    outlined in ``color``, its 1-based index written at the reference's label position in ``label_color``; the strings of ``texts`` are
    never rendered, they only bound the number of pairs (zip), ``None`` = every box.  ``image``: RGB uint8 HxWx3, numpy or tensor, host or
    device (a grey or otherwise shaped page: ValueError).  Returns a new device tensor; ``image`` is not modified.
    The pixels follow the library's own integer rule (include/ocrvi.h, "Result overlay": segments of thickness 1..15 with round caps, a
    seven-stroke digit font) and equal tests/overlay_ref.py bit for bit; cv2.drawContours / cv2.putText parity is unpinned (cv2 and its
    Hershey glyphs are absent).  Page sides up to 16384, vertices within +-16384."""
    return draw_boxes_pages([image], [boxes], None if texts is None else [texts], color, label_color, thickness, device)[0]


def save_result(path: str, image, boxes, texts=None, quality: int = 95, device: str = "cuda:0", format=None) -> bool:
    """The reference's ``--save_result`` (pipeline2.py:358-360 + :397-400): ``draw_boxes_with_text`` then ``imwrite``; only the file's
    bytes leave the device -- JPEG, or with ``format="png"`` a PNG, which keeps the thin outlines exact.  Returns what ``imwrite`` returns."""
    _check_format(format, "save_result")
    return imwrite(path, draw_boxes_with_text(image, boxes, texts, device=device), quality, device=device, format=format)


def detect_and_recognize(original_image, det_model, rec_model, post_processor: DBPostProcessor, device: str = "cuda:0", det_size: int = 640,
                         rec_size: Tuple[int, int] = (32, 256), rec_batch_size: int = 64, binary_head: bool = False, quad=None,
                         enhance: bool = False, crop: str = "rect", confidence: bool = False, beam: Optional[int] = None, nbest: int = 1,
                         lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
    """Steps 2 and 3 of the reference's per-image loop (pipeline2.py:306-352) with every stage on this library: resize + normalise on the
    device -> ``det_model`` -> ``post_processor`` on the host copy of the binary map -> boxes rescaled to the original image -> the
    bounding rectangle of each box cropped, resized and normalised on the device straight from the uploaded page -> ``rec_model`` greedy
    CTC in batches of ``rec_batch_size``.  ``original_image``: RGB uint8 HxWx3 (numpy or device tensor), or the bytes of a baseline JPEG or a PNG file
    (``bytes`` / ``bytearray`` / ``memoryview``: ``imdecode`` first, the reference's cv2.imread, pipeline2.py:284-288).
    ``binary_head``: call ``det_model.forward_binary`` (the binarise branch alone; same map in f32 / f16x2) instead of ``det_model(...)``.
    ``quad``: the document's four corners in ``original_image`` (step 1, pipeline2.py:291-302): the page is rectified first
    (``four_point_transform``) and replaces the original, so the boxes are in the rectified page's coordinates (:297).  ``quad="deskew"``:
    the page goes through ``deskew`` first (the skew estimated on the device, the page turned upright when it is tilted).
    ``enhance``: ``enhance_document`` on the (rectified) page before the detector resize (scanner.py:190-191): boxes and crops come from
    the enhanced page.
    ``crop``: ``"rect"`` (the reference's crop, the default) or ``"quad"``: each box's minimum-area rectangle is warped upright into the
    recogniser instead of its bounding rectangle (``quad_crops``, ``preprocess_crops_quad``); boxes and scores do not change.
    ``confidence=True``: the result gains a last element ``recs``, one ``rec.Recognition`` per box with ``recs[i].text == texts[i]``.
    ``beam=W``: ``texts`` stay the greedy strings; the result gains a last element (after ``recs`` when both are on), one list of
    ``rec.Hypothesis`` per box from the prefix beam search on the same forward's log-probabilities (best first, at most ``nbest``).
    ``lm=CharLM`` (only with ``beam``; ``lm_weight``, ``len_bonus``): that search with the language model fused in (``ocrvi_ctc_beam_lm``);
    the lists then hold ``rec.LMHypothesis``.
    Returns (rescaled_boxes [int32 (n_i, 2)], scores, texts); empty crops decode the all-zero tensor as pipeline2.py:154-156 does."""
    _check_crop(crop)
    check_beam(beam, nbest, rec_size[1] // 4)
    lm_kw = {}                                               # (without lm the recogniser is called as it always was)
    if lm is not None or lm_weight != 1.0 or len_bonus != 0.0:
        check_lm(lm, lm_weight, len_bonus, beam, rec_model.tokenizer.num_classes, rec_model.blank_id)
        lm_kw = dict(lm=lm, lm_weight=lm_weight, len_bonus=len_bonus)
    if isinstance(original_image, IMAGE_BYTES):              # a JPEG or PNG file's bytes: decoded on the device (``imdecode``)
        original_image = imdecode(original_image, device)
    page = original_image if isinstance(original_image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(original_image))
    page = page.to(device).contiguous()
    if isinstance(quad, str):
        if quad != "deskew":
            raise ValueError(f"quad: expected None, four corners or \"deskew\", got {quad!r}")
        page, quad = deskew(page)[0], None
    if quad is not None:
        page = four_point_transform(page, quad)
    if enhance:
        page = enhance_document(page)
    h, w = page.shape[:2]
    resized, (scale_h, scale_w) = resize_image_for_det(page, det_size)
    det_preds = det_model.forward_binary(normalize_for_det(resized)) if binary_head else det_model(normalize_for_det(resized))
    pred_binary = det_preds["binary"] if isinstance(det_preds, dict) else det_preds
    boxes, scores = post_processor(pred_binary[0])       # (copies the map to the host: the stream is synchronised from here on)
    if hasattr(det_model, "check_range"):
        det_model.check_range()                           # f16x2 only: OverflowError if an activation left fp16's range
    rescaled = rescale_boxes(boxes, scale_w, scale_h)
    texts: List[str] = []
    recs: List[Recognition] = []
    hyps: List[List[Hypothesis]] = []

    def decode(batch):
        if beam is not None:
            greedy, h = rec_model.decode_greedy_and_beam(batch, beam, nbest, confidence, **lm_kw)
            (recs if confidence else texts).extend(greedy)
            hyps.extend(h)
        elif confidence:
            recs.extend(rec_model.decode_greedy(batch, True))
        else:
            texts.extend(rec_model.decode_greedy(batch))

    def result():
        out = (rescaled, scores, [r.text for r in recs], recs) if confidence else (rescaled, scores, texts)
        return out + (hyps,) if beam is not None else out

    if crop == "quad":
        qc, qm = quad_crops(rescaled, (h, w))
        for i in range(0, len(qc), rec_batch_size):
            decode(preprocess_crops_quad(page[None], qc[i:i + rec_batch_size], qm[i:i + rec_batch_size], rec_size))
        return result()
    rects = [(0,) + crop_rect((h, w), b) for b in rescaled]
    for i in range(0, len(rects), rec_batch_size):
        chunk = rects[i:i + rec_batch_size]
        live = [r for r in chunk if r[3] > 0 and r[4] > 0]
        batch = torch.zeros((len(chunk), 3) + tuple(rec_size), device=page.device)
        if live:
            idx = torch.as_tensor([j for j, r in enumerate(chunk) if r[3] > 0 and r[4] > 0], device=page.device)
            batch[idx] = preprocess_crops(page[None], live, rec_size)
        decode(batch)
    return result()


def detect_and_recognize_pages(images, det_model, rec_model, post_processor: DBPostProcessor, device: str = "cuda:0", det_size: int = 640,
                               rec_size: Tuple[int, int] = (32, 256), rec_batch_size: int = 64, binary_head: bool = False, crop: str = "rect",
                               confidence: bool = False, beam: Optional[int] = None, nbest: int = 1,
                               lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
    """``detect_and_recognize`` for a list of pages of any sizes in one call: a one-shot ``engine.Engine`` (pages bucketed by detector
    shape, detector chunks and recogniser batches across pages).  ``det_model`` / ``rec_model`` are the library's DBNetPP / SVTRv2 on
    ``device``.  Returns [(rescaled_boxes, scores, texts) per page, in input order], each what ``detect_and_recognize`` returns for that
    page alone (``binary_head``, ``crop``, ``confidence``, ``beam``, ``nbest``, ``lm``, ``lm_weight`` and ``len_bonus`` as there; without
    ``beam`` the engine keeps no log-probabilities, so ``log_prob`` is ``None``)."""
    from .engine import Engine
    _check_crop(crop)
    if torch.device(device).type != "cuda" or _dev_index(device) != det_model._dev_index():
        raise ValueError(f"models live on cuda:{det_model._dev_index()}, not {device}")
    return Engine(det_model, rec_model, post_processor, det_size=det_size, rec_size=rec_size, rec_batch=rec_batch_size, binary_head=binary_head,
                  crop=crop, confidence=confidence, beam=beam, nbest=nbest, lm=lm, lm_weight=lm_weight, len_bonus=len_bonus).run(images)
