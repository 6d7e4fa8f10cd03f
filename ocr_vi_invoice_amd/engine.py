"""Batched OCR over pages of mixed sizes: the reference's per-image loop (src/pipeline/pipeline2.py:279-352) for a whole folder of
invoices at once, on the graph-replayed, two-stream path.

Pages are grouped into **buckets**: the pages that ``resize_image_for_det`` (pipeline2.py:33-40) maps to the same x32 detector shape.
A page is never padded into a larger shape (that would change the detector's output near its edges).  Each bucket runs through the
detector in chunks of up to ``det_chunk`` pages; the crops of every page of every bucket then share recogniser batches.

Per detector chunk, on the detector stream: the chunk's page table -> device, ``ocrvi_resize_normalize_pages`` + the detector's
``enqueue_forward`` (``ocrvi_det_forward``, binary map only; ``enqueue_forward_binary`` / ``ocrvi_det_forward_binary`` with
``binary_head=True``; one captured graph per (H, W, n), kept in an LRU of ``graph_cache``), the optional ``prob_hook``, the map -> a pinned
host slot of two, an event.  The host post-processes chunk c (``ocrvi_db_boxes_pages``) while the device runs chunk c + 1.  Rectangles
accumulate across chunks and buckets; each full ``rec_batch`` goes out on the recogniser stream: rectangles -> device,
``ocrvi_crop_resize_normalize_pages`` + the recogniser's ``enqueue_forward`` (``ocrvi_rec_forward``; one captured graph), ids / lens -> a
pinned host slot, an event.  The models' enqueue methods are the only call sites of the model entries: the engine passes its own
buffers and workspaces to them and never touches a handle.

Every result equals ``pipeline.detect_and_recognize`` run on that page alone in the f32 and f16x2 modes ("Batched engine":
in bf16 / f16 a kernel choice depends on the batch's row count, so a page inside a chunk may be computed differently from alone).
"""
from __future__ import annotations

import collections
import math
import os
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .codec import IMAGE_BYTES, JPEG, PNG, format_of_info, imdecode, info_struct, parse_into, stream_buffer, table_entry
from .pipeline import (DBPostProcessor, _check_crop, db_boxes_pages, enhance_init, enhance_workspace_bytes, estimate_skews, find_document_quads,
                       four_point_geometry, overlay_paint_, overlay_segments, quad_crops, skew_quad)
from .rec import check_beam, check_lm, make_recognitions

_ARENA_ALIGN = 256
_STREAMS: Dict[int, Tuple[torch.cuda.Stream, torch.cuda.Stream]] = {}


def plan_buckets(sizes: Sequence[Tuple[int, int]], det_size: int):
    """The detector shape of every page, with the reference's arithmetic (pipeline2.py:36-39): float64 ``scale = det_size / max(h, w)``,
    ``new = int(np.round(side * scale / 32) * 32)`` (round half to even: a 960 x 1280 page at det_size 960 gives 704 x 960).
    ``sizes``: (h, w) per page.  Returns (shapes [(new_h, new_w)], scales [(scale_h, scale_w)] = (new_h / h, new_w / w), buckets
    {(new_h, new_w): [page indices, in input order]} in order of first appearance).  A page whose side rounds to 0 raises ValueError
    naming it (cv2.resize raises there in the reference)."""
    shapes, scales, buckets = [], [], {}
    for i, hw in enumerate(sizes):
        h, w = int(hw[0]), int(hw[1])
        if h <= 0 or w <= 0:
            raise ValueError(f"page {i}: empty image ({h}x{w})")
        scale = det_size / max(h, w)
        new_h = int(np.round(h * scale / 32) * 32)
        new_w = int(np.round(w * scale / 32) * 32)
        if new_h <= 0 or new_w <= 0:
            raise ValueError(f"page {i}: {h}x{w} resizes to {new_h}x{new_w} at det_size {det_size} (a side rounds to 0; the reference's "
                             "cv2.resize rejects it)")
        shapes.append((new_h, new_w))
        scales.append((new_h / h, new_w / w))
        buckets.setdefault((new_h, new_w), []).append(i)
    return shapes, scales, buckets


def plan_rectified(sizes: Sequence[Tuple[int, int]], quads, det_size: int):
    """``plan_buckets`` for pages of which some are rectified first (``Engine.run(pages, quads)``): page i with ``quads[i]`` (four (x, y)
    corners, any order) is bucketed by the size ``four_point_transform`` (src/preprocess/scanner.py:29-53) gives it, a page with ``None`` by
    its own.  Host only.  Returns (rectified sizes [(h, w)], m_inv [None or float64 [9], destination -> source], shapes, scales, buckets),
    the last three as ``plan_buckets`` returns them for the rectified sizes.  ValueError naming the page for a quad that is not four finite
    (x, y) points or that the geometry refuses (``ocrvi_four_point_transform``: shorter than a pixel, degenerate after ordering)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    quads = [None] * len(sizes) if quads is None else list(quads)
    if len(quads) != len(sizes):
        raise ValueError(f"quads: {len(quads)} entries for {len(sizes)} pages")
    out_sizes, mats = [], []
    for i, (hw, q) in enumerate(zip(sizes, quads)):
        if q is None:
            out_sizes.append(hw)
            mats.append(None)
            continue
        _, m_inv, w, h = four_point_geometry(q, what=f"page {i}: quad")
        out_sizes.append((h, w))
        mats.append(m_inv.reshape(9))
    return (out_sizes, mats) + plan_buckets(out_sizes, det_size)


def _usable_cores(cap: int = 16) -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, cap))


class Engine:
    """``run(pages)`` -> [(boxes, scores, texts) per page, in input order], each exactly what ``pipeline.detect_and_recognize(page,
    det_model, rec_model, post_processor, det_size=det_size, rec_size=rec_size)`` returns for that page alone.

    ``det_model`` / ``rec_model``: the library's ``DBNetPP`` / ``SVTRv2`` (same device).  Defaults follow pipeline2's CLI (:212-220).
    ``max_pages`` pages are resident at a time in one device arena (a wave); ``graphs=False`` launches eagerly (same bits).
    ``prob_hook(prob, page_indices)``: called on the detector stream after each chunk's forward with the device map [n,1,H,W] (edit it in
    place) and the input indices of its pages -- how random-weight runs get a map with text structure.  It runs eagerly, outside the
    captured graphs.  ``post_threads``: host threads of the box stage (0 = the cores this process may use, at most 16).
    ``binary_head=True``: the detector runs ``ocrvi_det_forward_binary`` (the binarise branch alone; the same map in f32 / f16x2, about 8 % fewer
    detector FLOPs) with its own, never larger workspace; everything after the map is unchanged.
    ``run(pages, quads)``: ``quads[i]`` is ``None`` or the four corners of page i's document; such a page is rectified on the device
    (``ocrvi_warp_perspective_pages`` into its arena slot, ahead of its chunk's detector launch) and everything downstream sees the
    rectified page, as ``detect_and_recognize(page, ..., quad=quads[i])`` does: boxes are in its coordinates.
    ``run(pages, quads="auto")``: the corners are found first, by ``pipeline.find_document_quads`` (one page table and one launch per stage
    for all pages, on the current stream), then exactly the path above runs: the result equals ``run(pages, find_document_quads(pages),
    enhance)``.  Encoded pages are decoded once, up front (``codec.imdecode``), and host arrays uploaded once; they go on as device
    tensors, so ``stats`` counts no ``jpeg`` / ``png`` page in that mode.
    ``run(pages, quads="deskew")``: decoded and uploaded in the same way, the pages go through ``pipeline.estimate_skews`` (one page table
    and one launch per stage); a page whose estimate has ``k != 0`` and ``gain >= deskew_min_gain`` (the constructor's argument; 1.0 takes
    every non-zero estimate) gets ``pipeline.skew_quad(h, w, k)``, every other page ``None``, and the path above runs: the result equals
    ``run(pages, those_quads)``.  ``stats["deskewed"]`` counts the pages that were turned.
    ``run(pages, quads, enhance)``: ``enhance`` is a bool for all pages or one bool per page; such a page goes through
    ``ocrvi_enhance_u8`` (``pipeline.enhance_document``, src/preprocess/scanner.py:55-76) in its arena slot, after its rectification and
    ahead of its chunk's detector launch, eagerly on the detector stream, as ``detect_and_recognize(page, ..., enhance=True)`` does.
    ``crop="quad"``: the recogniser sees each box's minimum-area rectangle warped upright (``ocrvi_min_area_quads`` / ``ocrvi_quad_crops`` on
    the host after the box stage, ``ocrvi_crop_quad_resize_normalize_pages`` in the recogniser graph) instead of its bounding rectangle, as
    ``detect_and_recognize(page, ..., crop="quad")`` does; ``"rect"`` (the default) is the reference's crop.
    A page may also be the bytes of a baseline JPEG file (``bytes`` / ``bytearray`` / ``memoryview``; arrays and files mix freely): its
    size, after the EXIF orientation, comes from ``ocrvi_jpeg_info``; every file of the call is entropy-decoded on the host pool
    (``ocrvi_jpeg_parse``) before any device work, so a bad file raises ValueError naming its page and leaves nothing in flight; its
    coefficient stream goes through pinned staging with its chunk and ``ocrvi_jpeg_decode_pages`` decodes it straight into its arena
    slot (into the raw region when it has a quad), ahead of the chunk's warp and enhancement.  The results are those of the same page
    passed as the array ``pipeline.imdecode`` returns.  A page may equally be the bytes of a PNG file (told apart by its signature): its
    size comes from ``ocrvi_png_info``, it is inflated on the same host pool in the same stage (``ocrvi_png_parse``), its stream -- the
    filtered scanlines, for grey, palette and bilevel pages 1/3 to 1/24 of the RGB bytes -- goes through the same pinned staging, and one
    ``ocrvi_png_decode_pages`` launch per chunk decodes it into the same place.  ``stats`` counts ``jpeg`` / ``png`` pages, their
    ``*_stream_bytes`` and ``*_parse_s``.
    ``annotate=True`` (the constructor's argument, or the attribute set between runs; ``run``'s own parameters stay as they were): each
    page's result is a 4-tuple ``(boxes, scores, texts, annotated)``; ``annotated`` is a
    new device uint8 tensor: the page as the detector saw it (rectified and enhanced where asked for, as the reference draws on its
    preprocessed ``original_image``, pipeline2.py:358-360) with ``pipeline.draw_boxes_with_text(page, boxes, texts)`` painted on it -- per
    wave, one copy per page out of the arena and one ``ocrvi_overlay_pages`` launch.  The arena and the caller's tensors are never written.
    ``confidence=True`` (the constructor's argument only: it decides what the recogniser graph holds): each page's result gains a last
    element ``recs``, one ``rec.Recognition`` per box with ``recs[i].text == texts[i]`` (after ``annotated`` when both are on).  The
    recogniser graph then calls ``enqueue_forward_conf`` (``ocrvi_rec_forward_conf``) and ``char_lp`` / ``char_span`` come back beside the
    ids; no log-probabilities are stored, so ``log_prob`` is ``None``.  With ``False`` the engine enqueues exactly what it always has.
    ``beam=W, nbest=n`` (the constructor's arguments only, like ``confidence``; 1 <= n <= W <= 64): ``texts`` stay the greedy strings and
    each page's result gains a last element (after ``recs`` when both are on), one list of ``rec.Hypothesis`` per box, best first, at most
    ``n`` long.  The recogniser graph then keeps the forward's log-probabilities in a device buffer [T, rec_batch, C] and launches
    ``ocrvi_ctc_beam`` on them after the forward, on the same stream (a sequential node); ids / lens / score of the hypotheses come back
    through pinned slots beside the greedy ones.  With ``beam=None`` the engine enqueues exactly what it always has.
    ``lm=CharLM, lm_weight=a, len_bonus=b`` (the constructor's arguments only; legal only with ``beam``): ``ocrvi_ctc_beam_lm`` takes the
    place of the ``ocrvi_ctc_beam`` node, on the same stream, and the lists hold ``rec.LMHypothesis``; the two extra score arrays come
    back through pinned slots of their own.  The table is uploaded in the constructor, never inside a capture.  With ``lm=None`` the
    engine enqueues exactly what it enqueues without the argument.
    The captured graphs hold the models' weights as they were: after reloading a model's weights, build a new Engine."""

    def __init__(self, det_model, rec_model, post_processor: DBPostProcessor, det_size: int = 960, rec_size: Tuple[int, int] = (32, 256),
                 det_chunk: int = 16, rec_batch: int = 256, max_pages: int = 256, graphs: bool = True, graph_cache: int = 16,
                 post_threads: int = 0, prob_hook=None, binary_head: bool = False, crop: str = "rect", annotate: bool = False,
                 confidence: bool = False, beam: int = None, nbest: int = 1, lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0,
                 deskew_min_gain: float = 1.0):
        rh, rw = int(rec_size[0]), int(rec_size[1])
        if rh <= 0 or rw <= 0 or rh % 16 or rw % 4:
            raise ValueError(f"rec_size {rec_size}: the height must be a multiple of 16 and the width of 4")
        if det_size <= 0 or det_chunk <= 0 or rec_batch <= 0 or max_pages <= 0 or graph_cache <= 0:
            raise ValueError("det_size, det_chunk, rec_batch, max_pages and graph_cache must be positive")
        check_beam(beam, nbest, rw // 4)
        check_lm(lm, lm_weight, len_bonus, beam, rec_model.tokenizer.num_classes, rec_model.blank_id)
        self.det, self.rec, self.pp = det_model, rec_model, post_processor
        self.dev = det_model.device if det_model.device.index is not None else torch.device("cuda", det_model._dev_index())
        self.devi = det_model._dev_index()
        if rec_model._dev_index() != self.devi:
            raise ValueError(f"det_model is on cuda:{self.devi}, rec_model on cuda:{rec_model._dev_index()}")
        self.det_size, self.rec_size = int(det_size), (rh, rw)
        self.det_chunk, self.rec_batch, self.max_pages = int(det_chunk), int(rec_batch), int(max_pages)
        self.graphs, self.graph_cache, self.prob_hook = bool(graphs), int(graph_cache), prob_hook
        self.binary_head = bool(binary_head)
        self.deskew_min_gain = float(deskew_min_gain)
        self.crop = _check_crop(crop)
        self.post_threads = int(post_threads) or _usable_cores()
        self.lib = _lib.load()
        # every bucket det_size can produce fits in L x L (the longer side rounds to 32 round(det_size / 32); ceil covers a tie)
        self.L = L = 32 * int(math.ceil(det_size / 32))
        # the strided 1x1 layers and the 32-bit epilogue offsets of the ring GEMM switch kernels at n H W 64 bytes >= 2^32 (the widest
        # tensor: 256 fp32 / f16x2 channels at H/4 x W/4): a chunk past that would not compute what a page alone computes
        if self.det_chunk * L * L * 64 >= (1 << 32) - (1 << 20):
            raise ValueError(f"det_chunk {det_chunk} at det_size {det_size}: a {det_chunk}-page {L}x{L} chunk leaves the kernels a page alone "
                             "takes (n * L * L * 64 bytes must stay below 2^32); use a smaller det_chunk")
        d = dict(device=self.dev)
        # ---- detector: one workspace for every bucket shape at det_chunk (never the facade's per-shape cache, which frees the previous
        #      shape's buffer: a graph captured for one bucket would replay into freed memory)
        need = 0
        for s in range(32, L + 1, 32):
            for (h, w) in ((L, s), (s, L)):
                need = max(need, self._det_ws_bytes(self.det_chunk, h, w))
        self.det_ws = torch.empty(max(need, 1), dtype=torch.uint8, **d)
        self.d_x = torch.empty(self.det_chunk * 3 * L * L, dtype=torch.float32, **d)
        self.d_bin = torch.empty(self.det_chunk * L * L, dtype=torch.float32, **d)
        self.d_det_table = torch.zeros((self.det_chunk, _lib.PAGE_ENTRY), dtype=torch.int64, **d)
        self.h_map = [torch.empty(self.det_chunk * L * L, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.ev_map = [torch.cuda.Event() for _ in range(2)]
        # ---- recogniser: one batch shape, one workspace, one graph
        self.rec_ws = torch.empty(max(rec_model.workspace_bytes(self.rec_batch, rh, rw), 1), dtype=torch.uint8, **d)
        T = rw // 4
        self.d_rects = torch.zeros((self.rec_batch, 5), dtype=torch.int32, **d)
        self.d_crops = torch.empty((self.rec_batch, 3, rh, rw), dtype=torch.float32, **d)
        self.d_am = torch.empty((self.rec_batch, T), dtype=torch.int32, **d)
        self.d_ids = torch.empty((self.rec_batch, T), dtype=torch.int32, **d)
        self.d_lens = torch.empty((self.rec_batch,), dtype=torch.int32, **d)
        self.d_rec_table = torch.zeros((self.max_pages, _lib.PAGE_ENTRY), dtype=torch.int64, **d)
        nslots = 4
        self.h_rects = [torch.zeros((self.rec_batch, 5), dtype=torch.int32).pin_memory() for _ in range(nslots)]
        self.h_ids = [torch.empty((self.rec_batch, T), dtype=torch.int32).pin_memory() for _ in range(nslots)]
        self.h_lens = [torch.empty((self.rec_batch,), dtype=torch.int32).pin_memory() for _ in range(nslots)]
        self.ev_rec = [torch.cuda.Event() for _ in range(nslots)]
        self.confidence = bool(confidence)
        if self.confidence:                        # per-character records beside the ids: char_lp [B,T], char_span [B,T,2]
            self.d_char_lp = torch.empty((self.rec_batch, T), dtype=torch.float32, **d)
            self.d_char_span = torch.empty((self.rec_batch, T, 2), dtype=torch.int32, **d)
            self.h_char_lp = [torch.empty((self.rec_batch, T), dtype=torch.float32).pin_memory() for _ in range(nslots)]
            self.h_char_span = [torch.empty((self.rec_batch, T, 2), dtype=torch.int32).pin_memory() for _ in range(nslots)]
        self.beam, self.nbest = beam, int(nbest)
        self.lm, self.lm_weight, self.len_bonus = lm, float(lm_weight), float(len_bonus)
        if beam is not None:                       # the forward's log-probabilities stay on the device; the hypotheses come back
            C = rec_model.tokenizer.num_classes
            self.d_lp = torch.empty((T, self.rec_batch, C), dtype=torch.float32, **d)
            ws_bytes, shapes, self._enqueue_beam, self._make_hyps = rec_model._beam_search(T, self.rec_batch, beam, self.nbest, lm,
                                                                                           self.lm_weight, self.len_bonus)
            self.d_beam_ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, **d)
            if lm is not None:
                lm.to(self.dev)
            self.d_hyp = [torch.empty(sh, dtype=dt, **d) for sh, dt in shapes]         # ids, lens, score (with lm: ctc_score, lm_score)
            self.h_hyp = [[torch.empty(sh, dtype=dt).pin_memory() for sh, dt in shapes] for _ in range(nslots)]
        if self.crop == "quad":                    # oriented crops: a descriptor row (page, w, h, 0) and a matrix per crop instead of a rectangle
            self.d_qcrops = torch.zeros((self.rec_batch, 4), dtype=torch.int32, **d)
            self.d_qmat = torch.zeros((self.rec_batch, 9), dtype=torch.float64, **d)
            self.h_qcrops = [torch.zeros((self.rec_batch, 4), dtype=torch.int32).pin_memory() for _ in range(nslots)]
            self.h_qmat = [torch.zeros((self.rec_batch, 9), dtype=torch.float64).pin_memory() for _ in range(nslots)]
        # ---- pages: one device arena per wave, filled through pinned staging; the wave's page table (pinned, arena order)
        self.arena = torch.empty(0, dtype=torch.uint8, **d)
        self.h_stage = torch.empty(0, dtype=torch.uint8)
        self.h_table = torch.zeros((self.max_pages, _lib.PAGE_ENTRY), dtype=torch.int64).pin_memory()
        # ---- rectification (run(pages, quads)): per detector chunk, the raw pixels of its quad pages that came from the host (device region
        #      + two pinned slots, grown on demand) and one block of int64 words per chunk = source table | destination table | matrices
        self.d_raw = torch.empty(0, dtype=torch.uint8, **d)
        self.h_raw = [torch.empty(0, dtype=torch.uint8), torch.empty(0, dtype=torch.uint8)]
        words = self.det_chunk * (2 * _lib.PAGE_ENTRY + 9)
        self.d_warp = torch.zeros(words, dtype=torch.int64, **d)
        self.h_warp = [torch.zeros(words, dtype=torch.int64).pin_memory() for _ in range(2)]
        # ---- enhancement (run(pages, quads, enhance)): the workspace of the largest enhanced page and a page to enhance into (the entry
        #      refuses to work in place), grown per run
        self.d_enh_ws = torch.empty(0, dtype=torch.uint8, **d)
        self.d_enh_out = torch.empty(0, dtype=torch.uint8, **d)
        # ---- encoded pages: per detector chunk, the streams of its files (device region + two pinned slots, grown on demand) and the
        #      decoders' workspace (JPEG: the component planes of the chunk's files; PNG: the lines between bands), shared by the two
        #      formats; one decode table per format, their entries differ in width
        self.d_streams = torch.empty(0, dtype=torch.uint8, **d)
        self.h_streams = [torch.empty(0, dtype=torch.uint8), torch.empty(0, dtype=torch.uint8)]
        self.d_dec_ws = torch.empty(0, dtype=torch.uint8, **d)
        self.d_dec_tab = {f: torch.zeros((self.det_chunk, f.entry_width), dtype=torch.int64, **d) for f in (JPEG, PNG)}
        self.h_dec_tab = {f: [torch.zeros((self.det_chunk, f.entry_width), dtype=torch.int64).pin_memory() for _ in range(2)] for f in (JPEG, PNG)}
        # one stream pair per device for every engine of the process: each new HIP stream takes the next hardware queue round-robin
        if self.devi not in _STREAMS:
            _STREAMS[self.devi] = (torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev))
        self.s_det, self.s_rec = _STREAMS[self.devi]
        self._det_graphs: "collections.OrderedDict[tuple, torch.cuda.CUDAGraph]" = collections.OrderedDict()
        self._rec_graph = None
        self._rec_warm = False
        self._pool = None                          # host threads of the JPEG entropy decoder and of inflate, started with the first file
        self.annotate = bool(annotate)             # read at the start of every run; may be switched between runs
        self._annotate, self._annotated = False, []   # the running call's switch and its painted copies of the pages
        self.stats = {}

    # ------------------------------------------------------------------------------------------------ device work (enqueue-only)
    def _det_ws_bytes(self, n, h, w) -> int:
        return self.det.workspace_bytes(n, h, w, "binary" if self.binary_head else "forward")

    def _det_calls(self, n, H, W):
        st = self.s_det.cuda_stream
        _lib.check(self.lib.ocrvi_resize_normalize_pages(self.devi, self.d_det_table.data_ptr(), n, H, W, self.d_x.data_ptr(), st))
        x, out, ws = self.d_x.data_ptr(), self.d_bin.data_ptr(), self.det_ws
        if self.binary_head:
            self.det.enqueue_forward_binary(x, n, H, W, out, ws.data_ptr(), ws.numel(), st)
        else:
            self.det.enqueue_forward(x, n, H, W, (out, None, None, None, None), ws.data_ptr(), ws.numel(), st)

    def _rec_calls(self):
        st = self.s_rec.cuda_stream
        rh, rw = self.rec_size
        if self.crop == "quad":
            _lib.check(self.lib.ocrvi_crop_quad_resize_normalize_pages(self.devi, self.d_rec_table.data_ptr(), self.max_pages,
                                                                       self.d_qcrops.data_ptr(), self.d_qmat.data_ptr(), self.rec_batch, rh, rw,
                                                                       self.d_crops.data_ptr(), st))
        else:
            _lib.check(self.lib.ocrvi_crop_resize_normalize_pages(self.devi, self.d_rec_table.data_ptr(), self.max_pages, self.d_rects.data_ptr(),
                                                                  self.rec_batch, rh, rw, self.d_crops.data_ptr(), st))
        lp = self.d_lp.data_ptr() if self.beam is not None else None
        if self.confidence:
            self.rec.enqueue_forward_conf(self.d_crops.data_ptr(), self.rec_batch, rh, rw, lp, self.d_am.data_ptr(), self.d_ids.data_ptr(),
                                          self.d_lens.data_ptr(), None, self.d_char_lp.data_ptr(), self.d_char_span.data_ptr(),
                                          self.rec_ws.data_ptr(), self.rec_ws.numel(), st)
        else:
            self.rec.enqueue_forward(self.d_crops.data_ptr(), self.rec_batch, rh, rw, lp, self.d_am.data_ptr(), self.d_ids.data_ptr(),
                                     self.d_lens.data_ptr(), self.rec_ws.data_ptr(), self.rec_ws.numel(), st)
        if self.beam is not None:
            self._enqueue_beam(lp, [t.data_ptr() for t in self.d_hyp], self.d_beam_ws.data_ptr(), self.d_beam_ws.numel(), st)

    def _run_det(self, n, H, W):
        """Steps 2 and 3 of a chunk on the detector stream: the cached graph of (H, W, n), or an eager launch that is captured after it."""
        if not self.graphs:
            self._det_calls(n, H, W)
            return
        key = (H, W, n)
        g = self._det_graphs.get(key)
        if g is not None:
            self._det_graphs.move_to_end(key)
            g.replay()
            return
        self._det_calls(n, H, W)                  # first use: the real launch (also warms up what a capture must not do)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.s_det):   # (synchronises the device first: no evicted graph is still running below)
            self._det_calls(n, H, W)
        self._det_graphs[key] = g
        while len(self._det_graphs) > self.graph_cache:
            self._det_graphs.popitem(last=False)

    def _run_rec(self):
        if not self.graphs:
            self._rec_calls()
        elif self._rec_graph is not None:
            self._rec_graph.replay()
        else:
            self._rec_calls()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.s_rec):
                self._rec_calls()
            self._rec_graph = g

    # ------------------------------------------------------------------------------------------------ input
    @staticmethod
    def _check_page(i, p, info=None):
        if isinstance(p, IMAGE_BYTES):            # a JPEG file: its size after orientation; a PNG file: its size (ValueError naming the page)
            if info is None:
                info = info_struct(p, f"page {i}")
            return int(info.out_height), int(info.out_width)
        if isinstance(p, np.ndarray):
            ok = p.dtype == np.uint8
        elif isinstance(p, torch.Tensor):
            ok = p.dtype == torch.uint8
        else:
            raise ValueError(f"page {i}: expected an RGB uint8 HxWx3 numpy array or tensor, or JPEG or PNG bytes, got {type(p).__name__}")
        if not ok or p.ndim != 3 or p.shape[2] != 3:
            raise ValueError(f"page {i}: expected an RGB uint8 HxWx3 array, got dtype {p.dtype} shape {tuple(p.shape)}")
        return int(p.shape[0]), int(p.shape[1])

    def _parse_files(self, pages, infos):
        """Entropy-decodes every JPEG page and inflates every PNG page of the call on the engine's host pool (``post_threads`` threads,
        the budget of the box stage, which never runs at the same time): {page index: (info, uint8 stream, bytes used)}; the info is a
        ``JpegInfo`` or a ``PngInfo``.  ValueError naming the first bad page; nothing has touched the device by then.  ``jpeg_parse_s``
        and ``png_parse_s`` are the wall time from the start of this stage until the last file of that format was done (the two
        overlap when a call holds both).
        A stream waits in pageable memory until its chunk is staged and is dropped there.  It cannot be decoded into the pinned slot it
        is uploaded from: the two slots belong to the chunks in flight, while a corrupt scan must be found, for every file of the call,
        before the first chunk is launched; pinned room for a whole call would be hundreds of megabytes for a folder of pages.  The
        buffer is sized by the bound ``ocrvi_jpeg_info`` / ``ocrvi_png_info`` gives (``codec.stream_buffer``); only the pages the stream
        touches ever become resident."""
        if not infos:
            return {}
        t0 = time.perf_counter()

        def one(i):
            buf = stream_buffer(infos[i])
            used = parse_into(infos[i], pages[i], buf.ctypes.data, buf.nbytes, f"page {i}")
            return infos[i], buf, used, time.perf_counter()

        if self._pool is None:
            import concurrent.futures
            self._pool = concurrent.futures.ThreadPoolExecutor(self.post_threads, thread_name_prefix="ocrvi-codec")
        futs = [(i, self._pool.submit(one, i)) for i in sorted(infos)]
        out, err = {}, None
        for i, f in futs:                         # every job is waited for, the first failure in page order is raised
            try:
                info, buf, used, done = f.result()
                out[i] = (info, buf, used)
                key = f"{format_of_info(info).name}_parse_s"
                self.stats[key] = max(self.stats[key], done - t0)
            except Exception as e:               # noqa: BLE001
                err = err or e
        if err is not None:
            raise err
        return out

    def _decode_files(self, s, targets):
        """The JPEG and PNG pages of a chunk -> ``targets`` [(page index, destination address)], one ``decode_pages`` launch per format
        the chunk holds (JPEG first) on the detector stream: streams and tables through pinned slot ``s``; the two formats share the
        stream region and the workspace."""
        stage = self.h_streams[s].numpy()
        base = self.arena.data_ptr()
        count = {JPEG: 0, PNG: 0}
        tabs = {fmt: self.h_dec_tab[fmt][s].numpy() for fmt in count}
        soff = woff = 0
        for i, dst_ptr in targets:
            info, buf, used = self._encoded[i]
            fmt = format_of_info(info)
            stage[soff:soff + used] = buf[:used]
            self._encoded[i] = (info, None, used)  # the host copy has served: only its sizes are still read
            table_entry(info, used, soff, dst_ptr - base, 3 * info.out_width, woff, tabs[fmt][count[fmt]])
            count[fmt] += 1
            self.stats[f"{fmt.name}_stream_bytes"] += used
            soff += (used + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
            woff += info.workspace_bytes
        self.d_streams[:soff].copy_(self.h_streams[s][:soff], non_blocking=True)
        ws = self.d_dec_ws
        for fmt, n in count.items():
            if n:
                self.d_dec_tab[fmt][:n].copy_(self.h_dec_tab[fmt][s][:n], non_blocking=True)
                # (a chunk of PNG pages alone may need no workspace: a null pointer then)
                fmt.decode_pages(self.devi, self.d_streams.data_ptr(), self.d_dec_tab[fmt].data_ptr(), n, base,
                                 ws.data_ptr() if ws.numel() else None, ws.numel(), self.s_det.cuda_stream)
            self.stats[fmt.name] += n

    def _stage(self, pages, wave, lo, hi, s=0):
        """Pages wave[lo:hi] (consecutive arena slots) -> the arena, on the detector stream.  A page with a quad is warped into its slot
        (one ``ocrvi_warp_perspective_pages`` launch per chunk) from its raw pixels: a device page where it lies, a host page through
        pinned slot ``s`` and the raw region (chunk c - 2, the previous user of slot ``s``, has been waited for by now)."""
        PE, dc = _lib.PAGE_ENTRY, self.det_chunk
        tabs, roff, n_warp = None, 0, 0
        encoded = []                              # (page, destination address): the arena slot, or the raw region for a page with a quad
        for slot in range(lo, hi):
            i = wave[slot]
            p, off, nb = pages[i], self._offs[slot], self._nbytes[slot]
            dst = self.arena[off:off + nb]
            if self._mats[i] is not None:
                if tabs is None:
                    tabs = self.h_warp[s].numpy()
                    tabs[:] = 0                    # rows of pages without a quad stay invalid: the kernel skips them
                rh, rw = self._raw_sizes[i]
                if isinstance(p, torch.Tensor) and p.is_cuda:
                    src = p if p.is_contiguous() else p.contiguous()
                    self._keep.append(src)         # alive until the wave has drained
                    src_ptr = src.data_ptr()
                elif i in self._encoded:
                    src_ptr = self.d_raw.data_ptr() + roff
                    encoded.append((i, src_ptr))
                    roff += (rh * rw * 3 + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
                else:
                    src = p.numpy() if isinstance(p, torch.Tensor) else p
                    rb = rh * rw * 3
                    np.copyto(self.h_raw[s][roff:roff + rb].numpy().reshape(src.shape), src)
                    self.d_raw[roff:roff + rb].copy_(self.h_raw[s][roff:roff + rb], non_blocking=True)
                    src_ptr = self.d_raw.data_ptr() + roff
                    roff += (rb + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
                k = slot - lo
                tabs[k * PE:k * PE + PE] = (src_ptr, rh, rw, 0)
                tabs[(dc + k) * PE:(dc + k) * PE + PE] = (dst.data_ptr(), self._sizes[i][0], self._sizes[i][1], 0)
                tabs[2 * dc * PE + 9 * k:2 * dc * PE + 9 * k + 9] = self._mats[i].view(np.int64)
                n_warp += 1
            elif isinstance(p, torch.Tensor) and p.is_cuda:
                dst.copy_(p.contiguous().view(-1), non_blocking=True)
            elif i in self._encoded:
                encoded.append((i, dst.data_ptr()))
            else:
                src = p.numpy() if isinstance(p, torch.Tensor) else p
                stage = self.h_stage[off:off + nb].numpy()
                np.copyto(stage.reshape(src.shape), src)
                dst.copy_(self.h_stage[off:off + nb], non_blocking=True)
        if encoded:                                # ahead of the warp and the enhancement that read these pages
            self._decode_files(s, encoded)
        if n_warp:
            self.d_warp.copy_(self.h_warp[s], non_blocking=True)
            base = self.d_warp.data_ptr()
            _lib.check(self.lib.ocrvi_warp_perspective_pages(self.devi, base, base + dc * PE * 8, base + 2 * dc * PE * 8, hi - lo,
                                                             self.s_det.cuda_stream))
            self.stats["rectified"] += n_warp
        for slot in range(lo, hi):                 # after the upload / the warp of the page, on the same stream
            i = wave[slot]
            if not self._enhance[i]:
                continue
            (h, w), off, nb = self._sizes[i], self._offs[slot], self._nbytes[slot]
            _lib.check(self.lib.ocrvi_enhance_u8(self.devi, self.arena.data_ptr() + off, h, w, self.d_enh_out.data_ptr(), self.d_enh_ws.data_ptr(),
                                                 self.d_enh_ws.numel(), self.s_det.cuda_stream))
            self.arena[off:off + nb].copy_(self.d_enh_out[:nb], non_blocking=True)
            self.stats["enhanced"] += 1

    # ------------------------------------------------------------------------------------------------ recogniser batches
    def _launch_rec(self, rows, tags):
        if len(self._rec_inflight) == len(self.h_rects):
            self._decode_oldest()
        k = self._rec_slot
        self._rec_slot = (k + 1) % len(self.h_rects)
        if self.crop == "quad":                    # rows = (descriptor row, matrix) pairs
            hc, hm = self.h_qcrops[k].numpy(), self.h_qmat[k].numpy()
            hc[:len(rows)] = [r[0] for r in rows]
            hm[:len(rows)] = [r[1] for r in rows]
            hc[len(rows):] = 0                    # w = h = 0: the all-zero tensor; its string is dropped
            hm[len(rows):] = 0
        else:
            hr = self.h_rects[k].numpy()
            hr[:len(rows)] = rows
            hr[len(rows):] = 0                    # w = h = 0: the all-zero tensor; its string is dropped
        with torch.cuda.stream(self.s_rec):
            if self.crop == "quad":
                self.d_qcrops.copy_(self.h_qcrops[k], non_blocking=True)
                self.d_qmat.copy_(self.h_qmat[k], non_blocking=True)
            else:
                self.d_rects.copy_(self.h_rects[k], non_blocking=True)
            self._run_rec()
            self.h_ids[k].copy_(self.d_ids, non_blocking=True)
            self.h_lens[k].copy_(self.d_lens, non_blocking=True)
            if self.confidence:
                self.h_char_lp[k].copy_(self.d_char_lp, non_blocking=True)
                self.h_char_span[k].copy_(self.d_char_span, non_blocking=True)
            if self.beam is not None:
                for h, dv in zip(self.h_hyp[k], self.d_hyp):
                    h.copy_(dv, non_blocking=True)
            self.ev_rec[k].record(self.s_rec)
        self._rec_inflight.append((k, tags))
        self.stats["rec_batches"] += 1

    def _decode_oldest(self):
        k, tags = self._rec_inflight.popleft()
        t0 = time.perf_counter()
        self.ev_rec[k].synchronize()
        self.stats["rec_wait_s"] += time.perf_counter() - t0
        n = len(tags)
        if self.beam is not None:
            for (pg, b), h in zip(tags, self._make_hyps(self.rec.tokenizer, *[h[:n].numpy() for h in self.h_hyp[k]])):
                self._hyps[pg][b] = h
        if self.confidence:
            recs = make_recognitions(self.rec.tokenizer, self.h_ids[k][:n].numpy(), self.h_lens[k][:n].numpy(), self.h_char_lp[k][:n].numpy(),
                                     self.h_char_span[k][:n].numpy())
            for (pg, b), r in zip(tags, recs):
                self._texts[pg][b] = r.text
                self._recs[pg][b] = r
            return
        ids, lens = self.h_ids[k][:n].tolist(), self.h_lens[k][:n].tolist()
        texts = self.rec.tokenizer.decode([row[:m] for row, m in zip(ids, lens)])
        for (pg, b), t in zip(tags, texts):
            self._texts[pg][b] = t

    def _feed(self, rects, tags):
        self._pend_rects.extend(rects)
        self._pend_tags.extend(tags)
        rb = self.rec_batch
        while len(self._pend_rects) >= rb:
            self._launch_rec(self._pend_rects[:rb], self._pend_tags[:rb])
            del self._pend_rects[:rb], self._pend_tags[:rb]

    # ------------------------------------------------------------------------------------------------ detector chunks
    def _post(self, job):
        """Host stage of a launched chunk: wait for its map, ocrvi_db_boxes_pages, rectangles -> the recogniser queue."""
        idx, slots, (H, W), s = job
        n = len(idx)
        t0 = time.perf_counter()
        self.ev_map[s].synchronize()
        t1 = time.perf_counter()
        maps = self.h_map[s][:n * H * W].view(n, H, W)
        res = db_boxes_pages(maps, self.pp, [self._scales[i] for i in idx], [self._sizes[i] for i in idx], slots, threads=self.post_threads)
        self.stats["det_wait_s"] += t1 - t0
        self.stats["post_s"] += time.perf_counter() - t1
        rects, tags = [], []
        for i, slot, (polys, r, sc) in zip(idx, slots, res):
            self._boxes[i], self._scores[i] = polys, [float(v) for v in sc]
            self._texts[i] = [None] * len(polys)
            self._recs[i] = [None] * len(polys)
            self._hyps[i] = [None] * len(polys)
            if self.crop == "quad":                # the page's polygons -> quads -> descriptors, one batch call each
                tq = time.perf_counter()
                qc, qm = quad_crops(polys, self._sizes[i], page_id=slot)
                rects.extend(zip(qc.tolist(), qm))
                self.stats["quad_s"] += time.perf_counter() - tq
            else:
                rects.extend(r.tolist())
            tags.extend((i, b) for b in range(len(polys)))
        self.stats["crops"] += len(rects)
        self._feed(rects, tags)

    def _launch_det(self, pages, wave, lo, hi, shape, s):
        H, W = shape
        n = hi - lo
        idx = wave[lo:hi]
        t0 = time.perf_counter()
        with torch.cuda.stream(self.s_det):
            self._stage(pages, wave, lo, hi, s)
            self.d_det_table[:n].copy_(self.h_table[lo:hi], non_blocking=True)
            self._run_det(n, H, W)
            if self.prob_hook is not None:
                self.prob_hook(self.d_bin[:n * H * W].view(n, 1, H, W), list(idx))
            self.h_map[s][:n * H * W].copy_(self.d_bin[:n * H * W], non_blocking=True)
            self.ev_map[s].record(self.s_det)
        self.stats["launch_s"] += time.perf_counter() - t0
        return (idx, list(range(lo, hi)), shape, s)

    def _run_wave(self, pages, wave):
        # arena layout and page table of the wave (slots in bucket order, so every chunk is a run of consecutive slots)
        offs, nbytes, off = [], [], 0
        for i in wave:
            h, w = self._sizes[i]
            offs.append(off)
            nbytes.append(h * w * 3)
            off += (h * w * 3 + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
        self._offs, self._nbytes = offs, nbytes
        if self.arena.numel() < off:               # (the previous wave has drained: nothing reads the old arena any more)
            self.arena = torch.empty(off, dtype=torch.uint8, device=self.dev)
        on_host = [not (isinstance(pages[i], torch.Tensor) and pages[i].is_cuda) for i in wave]
        if any(h and self._mats[i] is None and i not in self._encoded for h, i in zip(on_host, wave)) and self.h_stage.numel() < off:
            self.h_stage = torch.empty(off, dtype=torch.uint8).pin_memory()
        tab = self.h_table.numpy()
        tab[:] = 0
        base = self.arena.data_ptr()
        for slot, i in enumerate(wave):
            tab[slot] = (base + offs[slot], self._sizes[i][0], self._sizes[i][1], 0)
        with torch.cuda.stream(self.s_rec):
            self.d_rec_table.copy_(self.h_table, non_blocking=True)
        # chunks: consecutive slots of one shape, at most det_chunk of them
        chunks, lo = [], 0
        while lo < len(wave):
            shape = self._shapes[wave[lo]]
            hi = lo + 1
            while hi < len(wave) and hi - lo < self.det_chunk and self._shapes[wave[hi]] == shape:
                hi += 1
            chunks.append((lo, hi, shape))
            lo = hi
        # the raw region: the largest chunk's host pages with a quad (per chunk, not per wave: 256 raw 12-megapixel pages would be 9 GB)
        raw = 0
        for lo, hi, _ in chunks:
            raw = max(raw, sum((self._raw_sizes[wave[k]][0] * self._raw_sizes[wave[k]][1] * 3 + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
                               for k in range(lo, hi) if on_host[k] and self._mats[wave[k]] is not None))
        if self.d_raw.numel() < raw:               # (the previous wave has drained)
            self.d_raw = torch.empty(raw, dtype=torch.uint8, device=self.dev)
            self.h_raw = [torch.empty(raw, dtype=torch.uint8).pin_memory() for _ in range(2)]
        # the regions of the encoded pages: the largest chunk's streams and decoder workspaces
        streams = dec_ws = 0
        for lo, hi, _ in chunks:
            files = [self._encoded[wave[k]] for k in range(lo, hi) if wave[k] in self._encoded]
            streams = max(streams, sum((u + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN for _, _, u in files))
            dec_ws = max(dec_ws, sum(info.workspace_bytes for info, _, _ in files))
        if self.d_streams.numel() < streams:       # (the previous wave has drained)
            self.d_streams = torch.empty(streams, dtype=torch.uint8, device=self.dev)
            self.h_streams = [torch.empty(streams, dtype=torch.uint8).pin_memory() for _ in range(2)]
        if self.d_dec_ws.numel() < dec_ws:
            self.d_dec_ws = torch.empty(dec_ws, dtype=torch.uint8, device=self.dev)
        pending = collections.deque()
        for c, (lo, hi, shape) in enumerate(chunks):
            if len(pending) == 2:                  # its pinned map slot is the one chunk c reuses
                self._post(pending.popleft())
            pending.append(self._launch_det(pages, wave, lo, hi, shape, c & 1))
        while pending:
            self._post(pending.popleft())
        # drain the wave: the last partial recogniser batch goes out padded, every string is decoded
        if self._pend_rects:
            self._launch_rec(self._pend_rects, self._pend_tags)
            self._pend_rects, self._pend_tags = [], []
        while self._rec_inflight:
            self._decode_oldest()
        self.s_det.synchronize()
        self.s_rec.synchronize()                   # (the table upload, even when the wave produced no crop)
        if self._annotate:
            self._annotate_wave(wave)
        self._keep = []

    def _annotate_wave(self, wave):
        """``annotate=True``: every page of the drained wave is copied out of the arena into a tensor of its own, and all copies
        are painted with the wave's boxes and region numbers by one ``ocrvi_overlay_pages`` launch (``pipeline.draw_boxes_pages`` without
        its upload of pixels), on the caller's stream.  Nothing writes the arena; the next wave reuses it, so the copies are waited for."""
        outs = []
        for slot, i in enumerate(wave):
            (h, w), off, nb = self._sizes[i], self._offs[slot], self._nbytes[slot]
            outs.append(self.arena[off:off + nb].clone().view(h, w, 3))
        overlay_paint_(outs, *overlay_segments([self._boxes[i] for i in wave], [self._texts[i] for i in wave], [self._sizes[i] for i in wave]))
        torch.cuda.current_stream(self.dev).synchronize()
        for i, out in zip(wave, outs):
            self._annotated[i] = out

    # ------------------------------------------------------------------------------------------------ public
    def run(self, pages: Sequence, quads: Sequence = None, enhance=None) -> List[Tuple[list, list, list]]:
        pages = list(pages)
        self._annotate, self._annotated = bool(self.annotate), [None] * len(pages)
        t_start = time.perf_counter()              # (total_s includes the host entropy decode of JPEG pages and the inflate of PNG pages)
        deskewed = 0
        if isinstance(quads, str):
            if quads not in ("auto", "deskew"):
                raise ValueError(f"quads: expected None, a list of quads, \"auto\" or \"deskew\", got {quads!r}")
            for i, p in enumerate(pages):
                self._check_page(i, p)
            enc = [i for i, p in enumerate(pages) if isinstance(p, IMAGE_BYTES)]
            for i, page in zip(enc, imdecode([pages[i] for i in enc], self.dev) if enc else []):
                pages[i] = page
            pages = [p if isinstance(p, torch.Tensor) and p.is_cuda else
                     torch.as_tensor(np.ascontiguousarray(p) if isinstance(p, np.ndarray) else p).to(self.dev) for p in pages]
            if quads == "auto":
                quads = find_document_quads(pages, device=self.dev)
            else:
                skews = estimate_skews(pages, device=self.dev)
                quads = [skew_quad(p.shape[0], p.shape[1], s.k) if s is not None and s.k != 0 and s.gain >= self.deskew_min_gain else None
                         for p, s in zip(pages, skews)]
                deskewed = sum(q is not None for q in quads)
        infos = {i: info_struct(p, f"page {i}") for i, p in enumerate(pages) if isinstance(p, IMAGE_BYTES)}
        raw_sizes = [self._check_page(i, p, infos.get(i)) for i, p in enumerate(pages)]
        # (every ValueError -- pages, quads, sizes that round to 0 -- is raised here, before any GPU work)
        sizes, mats, shapes, scales, buckets = plan_rectified(raw_sizes, quads, self.det_size)
        if enhance is None or isinstance(enhance, (bool, np.bool_)):
            flags = [bool(enhance)] * len(pages)
        else:
            flags = [bool(e) for e in enhance]
            if len(flags) != len(pages):
                raise ValueError(f"enhance: {len(flags)} entries for {len(pages)} pages")
        enh_ws = enh_out = 0
        for i, ((h, w), e) in enumerate(zip(sizes, flags)):
            if e:
                if h < _lib.ENHANCE_MIN_SIDE or w < _lib.ENHANCE_MIN_SIDE:
                    raise ValueError(f"page {i}: enhance needs both sides >= {_lib.ENHANCE_MIN_SIDE}, the page is {h}x{w}")
                enh_ws, enh_out = max(enh_ws, enhance_workspace_bytes(h, w)), max(enh_out, h * w * 3)
        for i, (h, w) in enumerate(shapes):
            if h > self.L or w > self.L:
                raise RuntimeError(f"page {i}: bucket {h}x{w} exceeds the {self.L}x{self.L} the workspace was sized for")
        self.stats = {"pages": len(pages), "buckets": {f"{h}x{w}": len(v) for (h, w), v in buckets.items()}, "crops": 0, "rec_batches": 0,
                      "rectified": 0, "enhanced": 0, "deskewed": deskewed, "launch_s": 0.0, "det_wait_s": 0.0, "post_s": 0.0, "rec_wait_s": 0.0}
        if self.crop == "quad":
            self.stats["quad_s"] = 0.0             # host time of ocrvi_min_area_quads + ocrvi_quad_crops (not part of post_s)
        if not pages:
            return []
        for fmt in (JPEG, PNG):
            self.stats.update({fmt.name: 0, f"{fmt.name}_stream_bytes": 0, f"{fmt.name}_parse_s": 0.0})
        self._encoded = self._parse_files(pages, infos)      # (a corrupt scan raises here: still before any GPU work)
        self._sizes, self._shapes, self._scales = sizes, shapes, scales
        self._raw_sizes, self._mats, self._keep = raw_sizes, mats, []
        self._enhance = flags
        if enh_ws:                                 # (the previous run has drained: nothing uses the old buffers any more)
            enhance_init(self.devi)
            if self.d_enh_ws.numel() < enh_ws:
                self.d_enh_ws = torch.empty(enh_ws, dtype=torch.uint8, device=self.dev)
            if self.d_enh_out.numel() < enh_out:
                self.d_enh_out = torch.empty(enh_out, dtype=torch.uint8, device=self.dev)
        self._boxes, self._scores, self._texts = [None] * len(pages), [None] * len(pages), [None] * len(pages)
        self._recs = [None] * len(pages)
        self._hyps = [None] * len(pages)
        self._pend_rects, self._pend_tags = [], []
        self._rec_inflight, self._rec_slot = collections.deque(), 0
        order = [i for v in buckets.values() for i in v]
        cur = torch.cuda.current_stream(self.dev)
        self.s_det.wait_stream(cur)                # device pages the caller just produced
        self.s_rec.wait_stream(cur)
        _lib.check(self.lib.ocrvi_range_reset(self.devi, self.s_det.cuda_stream))
        self.s_rec.wait_stream(self.s_det)
        try:
            for w0 in range(0, len(order), self.max_pages):
                self._run_wave(pages, order[w0:w0 + self.max_pages])
        finally:
            self.s_det.synchronize()
            self.s_rec.synchronize()
        rc = self.det.range_status()
        if rc == 0:
            rc = self.rec.range_status()
        if rc != 0:
            msg = _lib.last_error()
            _lib.check(self.lib.ocrvi_range_reset(self.devi, self.s_det.cuda_stream))
            self.s_det.synchronize()
            if rc == -5:
                raise OverflowError(msg)
            _lib.check(rc)
        self.stats["total_s"] = time.perf_counter() - t_start
        out = [(self._boxes[i], self._scores[i], self._texts[i]) for i in range(len(pages))]
        if self._annotate:
            annotated, self._annotated = self._annotated, []
            out = [r + (annotated[i],) for i, r in enumerate(out)]
        if self.confidence:
            out = [r + (self._recs[i],) for i, r in enumerate(out)]
        if self.beam is not None:
            out = [r + (self._hyps[i],) for i, r in enumerate(out)]
        return out
