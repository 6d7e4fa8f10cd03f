"""File I/O on top of libocrvi: everything that turns the bytes of an image file into pages and pages into the bytes of a file.

Reading is the reference's ``cv2.imread`` + ``cvtColor(BGR2RGB)`` (src/pipeline/pipeline2.py:284-288): ``imdecode`` / ``imread`` for baseline
JPEG and PNG.  The two decode formats are described once (``Format``: ``JPEG`` and ``PNG``) and every host wrapper of their entries --
header, stream, table entry, batched launch -- is written once on top of that description; ``jpeg_*`` / ``png_*`` bind them to one format.
Writing is the reference's ``cv2.imwrite`` (pipeline2.py:397-400): ``imencode`` / ``imencode_pages`` (baseline JPEG), ``imencode_png`` /
``imencode_png_pages`` and ``imwrite``; ``JpegEncodeJob`` and ``PngEncodeJob`` are the batched jobs behind them and share one base class.
``pipeline`` re-exports the public names; ``engine`` stages encoded pages with the same wrappers.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import ctypes

import numpy as np
import torch

from . import _lib


def _dev_index(device) -> int:
    d = torch.device(device)
    return d.index if d.index is not None else torch.cuda.current_device()


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


IMAGE_BYTES = (bytes, bytearray, memoryview)      # what an encoded page may be: the bytes of a baseline JPEG file or of a PNG file
JPEG_BYTES = IMAGE_BYTES
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_POOL = None


def host_pool():
    """The host thread pool of the per-file stages (the entries hold no lock and ctypes releases the interpreter lock)."""
    global _POOL
    if _POOL is None:
        import concurrent.futures
        import os
        try:
            n = len(os.sched_getaffinity(0))
        except AttributeError:
            n = os.cpu_count() or 1
        _POOL = concurrent.futures.ThreadPoolExecutor(max(1, min(n, 16)), thread_name_prefix="ocrvi-codec")
    return _POOL


def _bytes_view(data) -> np.ndarray:
    """The file's bytes as a uint8 array, without a copy."""
    if not isinstance(data, IMAGE_BYTES):
        raise ValueError(f"expected JPEG bytes (bytes, bytearray or memoryview), got {type(data).__name__}")
    return np.frombuffer(data, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- decode
class Format(NamedTuple):
    """One decode format: its name (also the prefix of its ``Engine.stats`` keys), its ``_lib`` info struct, the names of its four C
    entries and the int64 width of its table entry.  The methods are the host wrappers of those entries, the same for every format."""
    name: str
    info: type
    c_info: str
    c_parse: str
    c_table_entry: str
    c_decode_pages: str
    entry_width: int

    def info_struct(self, data, what: Optional[str] = None):
        """``ocrvi_*_info`` (host only); ValueError ``what: message`` for a file the library refuses or cannot read."""
        a = _bytes_view(data)
        info = self.info()
        rc = getattr(_lib.load(), self.c_info)(a.ctypes.data if a.size else None, a.size, ctypes.byref(info))
        if rc == -1:
            raise ValueError(f"{self.name if what is None else what}: {info.reason.decode('utf-8', 'replace')}")
        _lib.check(rc)
        return info

    def parse_into(self, data, out_ptr: int, cap: int, what: Optional[str] = None) -> int:
        """``ocrvi_*_parse`` into ``cap`` bytes at ``out_ptr``; returns the bytes used.  The error is read on the calling thread (it is
        thread-local): ValueError for a corrupt file, MemoryError for a short buffer."""
        a = _bytes_view(data)
        used = ctypes.c_size_t()
        rc = getattr(_lib.load(), self.c_parse)(a.ctypes.data if a.size else None, a.size, out_ptr, cap, ctypes.byref(used))
        if rc == -1:
            raise ValueError(f"{self.name if what is None else what}: {_lib.last_error()}")
        _lib.check(rc)
        return used.value

    def table_entry(self, info, used: int, stream_offset: int, dst_offset: int, dst_stride: int, workspace_offset: int, entry: np.ndarray) -> None:
        """``ocrvi_*_table_entry`` into ``entry`` (int64 [entry_width], contiguous)."""
        assert entry.dtype == np.int64 and entry.size == self.entry_width and entry.flags.c_contiguous
        _lib.check(getattr(_lib.load(), self.c_table_entry)(ctypes.byref(info), used, stream_offset, dst_offset, dst_stride, workspace_offset,
                                                            entry.ctypes.data))

    def decode_pages(self, devi: int, streams: int, table: int, n: int, dst: int, workspace, workspace_bytes: int, stream) -> None:
        """``ocrvi_*_decode_pages``: one batched launch for ``n`` table entries (device addresses; ``workspace`` may be None when no
        entry needs one)."""
        _lib.check(getattr(_lib.load(), self.c_decode_pages)(devi, streams, table, n, dst, workspace, workspace_bytes, stream))

    def parse(self, data) -> np.ndarray:
        """The stream of a file as the uint8 bytes ``ocrvi_*_parse`` wrote (host only; include/ocrvi.h states the formats)."""
        buf = stream_buffer(self.info_struct(data))
        return buf[:self.parse_into(data, buf.ctypes.data, buf.nbytes)]


JPEG = Format("jpeg", _lib.JpegInfo, "ocrvi_jpeg_info", "ocrvi_jpeg_parse", "ocrvi_jpeg_table_entry", "ocrvi_jpeg_decode_pages", _lib.JPEG_ENTRY)
PNG = Format("png", _lib.PngInfo, "ocrvi_png_info", "ocrvi_png_parse", "ocrvi_png_table_entry", "ocrvi_png_decode_pages", _lib.PNG_ENTRY)


def format_of(data) -> Format:
    """``PNG`` for ``data`` (``IMAGE_BYTES``) that starts with the PNG signature; everything else is handed to the JPEG decoder, whose
    messages name what is wrong with it."""
    return PNG if isinstance(data, IMAGE_BYTES) and _bytes_view(data)[:8].tobytes() == PNG_SIGNATURE else JPEG


def format_of_info(info) -> Format:
    """The format whose ``info_struct`` returned ``info``."""
    return PNG if isinstance(info, PNG.info) else JPEG


def is_png(data) -> bool:
    """Whether ``format_of(data)`` is ``PNG``."""
    return format_of(data) is PNG


def info_struct(data, what: Optional[str] = None):
    """``Format.info_struct`` of the format the file's signature names: a ``JpegInfo`` or a ``PngInfo``."""
    return format_of(data).info_struct(data, what)


def parse_into(info, data, out_ptr: int, cap: int, what: Optional[str] = None) -> int:
    """``Format.parse_into`` of the format ``info`` belongs to."""
    return format_of_info(info).parse_into(data, out_ptr, cap, what)


def table_entry(info, *args) -> None:
    """``Format.table_entry`` of the format ``info`` belongs to."""
    format_of_info(info).table_entry(info, *args)


def stream_buffer(info) -> np.ndarray:
    """Pageable room for the stream of ``info``'s file: uint8 [stream_bytes], the bound ``ocrvi_*_info`` gives, on a 4-byte boundary
    (the JPEG stream is uint32 words)."""
    return np.empty((info.stream_bytes + 3) // 4, np.uint32).view(np.uint8)[:info.stream_bytes]


jpeg_info_struct, jpeg_parse_into, jpeg_table_entry = JPEG.info_struct, JPEG.parse_into, JPEG.table_entry
png_info_struct, png_parse_into, png_table_entry, png_parse = PNG.info_struct, PNG.parse_into, PNG.table_entry, PNG.parse


def jpeg_parse(data) -> np.ndarray:
    """The sparse coefficient stream of a file as uint32 words (host only; include/ocrvi.h states the format)."""
    return JPEG.parse(data).view(np.uint32).copy()


def jpeg_info(data) -> dict:
    """What ``ocrvi_jpeg_info`` reports about a JPEG file (host only, needs no GPU): the coded width, height, components, sampling factors,
    restart interval, EXIF orientation, the decoded page's ``out_height`` / ``out_width`` (after orientation), the number of blocks and the
    two sizes ``stream_bytes`` / ``workspace_bytes``.  ValueError naming the feature for an unsupported file, or the fault of a corrupt one."""
    info = jpeg_info_struct(data)
    n = info.components
    return {"width": info.width, "height": info.height, "components": n, "h_samp": list(info.h_samp)[:n], "v_samp": list(info.v_samp)[:n],
            "restart_interval": info.restart_interval, "orientation": info.orientation, "out_height": info.out_height,
            "out_width": info.out_width, "blocks": info.blocks, "stream_bytes": info.stream_bytes, "workspace_bytes": info.workspace_bytes,
            "quant": np.ctypeslib.as_array(info.quant).copy()[:n]}


def png_info(data) -> dict:
    """What ``ocrvi_png_info`` reports about a PNG file (host only, needs no GPU).  ValueError naming the feature for an unsupported
    file, or the fault of a corrupt one."""
    info = png_info_struct(data)
    return {k: getattr(info, k) for k in ("width", "height", "bit_depth", "colour_type", "channels", "row_bytes", "out_height", "out_width",
                                          "palette_entries", "idat_bytes", "stream_bytes", "workspace_bytes")}


def png_plan(info) -> dict:
    """``ocrvi_png_plan`` (host only): ``band_rows``, ``chunk_bytes``, ``bands`` and ``steps`` of the kernel's walk over the page."""
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().ocrvi_png_plan(ctypes.byref(info), *[ctypes.byref(x) for x in v]))
    return dict(zip(("band_rows", "chunk_bytes", "bands", "steps"), (x.value for x in v)))


def _imdecode_group(fmt: Format, files, infos, names, dev):
    """The files of one format -> pages, in one batched launch (``Format.decode_pages``)."""
    s_off, w_off, d_off = [0], [0], [0]
    for info in infos:
        s_off.append(s_off[-1] + _align(info.stream_bytes))
        w_off.append(w_off[-1] + info.workspace_bytes)
        d_off.append(d_off[-1] + _align(info.out_height * info.out_width * 3))
    h_rec = torch.empty(s_off[-1], dtype=torch.uint8).pin_memory()
    base = h_rec.data_ptr()
    jobs = [(f, base + s_off[i], infos[i].stream_bytes, names[i]) for i, f in enumerate(files)]
    if len(files) > 1:
        used = list(host_pool().map(lambda j: fmt.parse_into(*j), jobs))
    else:
        used = [fmt.parse_into(*jobs[0])]
    table = np.zeros((len(files), fmt.entry_width), np.int64)
    for i, info in enumerate(infos):
        fmt.table_entry(info, used[i], s_off[i], d_off[i], 3 * info.out_width, w_off[i], table[i])
    with torch.cuda.device(dev):
        d_rec = torch.empty(s_off[-1], dtype=torch.uint8, device=dev)
        for i in range(len(files)):            # only the bytes each stream uses cross the bus
            d_rec[s_off[i]:s_off[i] + used[i]].copy_(h_rec[s_off[i]:s_off[i] + used[i]], non_blocking=True)
        d_tab = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
        ws = torch.empty(max(w_off[-1], 8), dtype=torch.uint8, device=dev)
        out = torch.empty(d_off[-1], dtype=torch.uint8, device=dev)
        fmt.decode_pages(_dev_index(dev), d_rec.data_ptr(), d_tab.data_ptr(), len(files), out.data_ptr(), ws.data_ptr(), ws.numel(),
                         torch.cuda.current_stream(dev).cuda_stream)
    return [out[d_off[i]:d_off[i] + info.out_height * info.out_width * 3].view(info.out_height, info.out_width, 3)
            for i, info in enumerate(infos)]


def imdecode(data, device: str = "cuda:0"):
    """cv2.imdecode / cv2.imread + cvtColor(BGR2RGB) (src/pipeline/pipeline2.py:284-288) for baseline JPEG and PNG: ``data`` is the bytes
    of one file (-> one uint8 [h, w, 3] RGB tensor on ``device``) or a list of them (-> a list of tensors in the caller's order).  The
    decoder is chosen per file by its signature (the PNG signature against FF D8); a list may mix the two formats and costs one batched
    launch per format.  What is serial per file runs on the host, a thread per file (JPEG: entropy decoding; PNG: inflate), everything else
    in ``ocrvi_jpeg_decode_pages`` / ``ocrvi_png_decode_pages`` on the current stream; a JPEG's EXIF orientation is applied.  ValueError for
    an unsupported or corrupt file (naming its index in a list); there is no host decoder behind these.  The arithmetic is stated in
    include/ocrvi.h: PIL's output for encoder-produced JPEG files and for PNG (16-bit grey aside), cv2 parity unpinned."""
    single = isinstance(data, IMAGE_BYTES)
    files = [data] if single else list(data)
    if not files:
        return []
    names = ["imdecode" if single else f"imdecode: file {i}" for i in range(len(files))]
    dev = torch.device(device)
    # every header is read (a bad one named, in the caller's order) before anything is decoded
    infos = [info_struct(f, name) for f, name in zip(files, names)]
    pages = [None] * len(files)
    for fmt in (JPEG, PNG):
        group = [i for i, info in enumerate(infos) if format_of_info(info) is fmt]
        if group:
            decoded = _imdecode_group(fmt, [files[i] for i in group], [infos[i] for i in group], [names[i] for i in group], dev)
            for i, page in zip(group, decoded):
                pages[i] = page
    return pages[0] if single else pages


def imread(path: str, device: str = "cuda:0") -> torch.Tensor:
    """``cv2.imread(path)`` + ``cvtColor(BGR2RGB)`` of the reference's loop (pipeline2.py:284-288) for a baseline JPEG or a PNG file: the file's
    bytes through ``imdecode``.  OSError for an unreadable file (the reference gets ``None`` and skips the image), ValueError for one that
    is neither a supported JPEG nor a supported PNG."""
    with open(path, "rb") as f:
        return imdecode(f.read(), device)


# ---------------------------------------------------------------------------------------------------- encode
class _EncodeJob:
    """The pages of one ``ocrvi_*_encode_pages`` call: validated and laid out by the constructor (ValueError before anything touches
    the device), uploaded and enqueued by ``launch`` (one page table, one set of launches, no synchronisation), read back by ``collect``
    (the lengths, then only the compressed bytes).  A format gives ``_name``, ``_entry_width``, ``_c_encode_pages`` and the hooks
    ``_geom``, ``_sizes`` and ``_table_entry``; its constructor sets what they read before it calls this one."""
    _name = _entry_width = _c_encode_pages = None

    def __init__(self, images, device, what: str):
        self.images = list(images)
        self.dev = torch.device(device)
        self.geom = []
        for i, im in enumerate(self.images):
            if not isinstance(im, (np.ndarray, torch.Tensor)):
                raise ValueError(f"{what}: page {i}: expected a numpy array or a tensor, got {type(im).__name__}")
            if im.dtype not in (np.uint8, torch.uint8):
                raise ValueError(f"{what}: page {i}: dtype {im.dtype} (uint8 expected)")
            shape = tuple(im.shape)
            if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
                raise ValueError(f"{what}: page {i}: shape {shape} (H x W x 3 RGB or H x W grey expected)")
            if not (1 <= shape[0] <= 65500 and 1 <= shape[1] <= 65500):
                raise ValueError(f"{what}: page {i}: sides {shape[0]} x {shape[1]} outside 1..65500")
            self.geom.append(self._geom(shape[0], shape[1], 1 if len(shape) == 2 else 3))
        self.w_off, self.o_off, self.caps = [0], [0], []
        for i, g in enumerate(self.geom):      # _sizes is called once per page, in page order: a format may record per-page results in it
            rc, wsb, cap = self._sizes(i, *g[:3])
            if rc == -1:
                raise ValueError(f"{what}: page {i}: {_lib.last_error()}")
            _lib.check(rc)
            self.caps.append(_align(cap))
            self.w_off.append(self.w_off[-1] + wsb)
            self.o_off.append(self.o_off[-1] + self.caps[-1])
        self.lengths = self.out = None

    def _geom(self, h: int, w: int, nc: int) -> tuple:
        """The ``geom`` entry of a validated page; it starts with (h, w, components)."""
        return h, w, nc

    def _sizes(self, i: int, h: int, w: int, nc: int) -> Tuple[int, int, int]:
        """``ocrvi_*_encode_sizes`` for page i: (return code, workspace bytes, output capacity)."""
        raise NotImplementedError

    def _table_entry(self, i: int, src_offset: int, row_bytes: int, entry: np.ndarray) -> None:
        """``ocrvi_*_encode_table_entry`` for page i into ``entry`` (a row of the page table)."""
        raise NotImplementedError

    def launch(self):
        n = len(self.images)
        if n == 0:
            return self
        dev = self.dev
        with torch.cuda.device(dev):
            # host pages travel in one pinned buffer and one copy; device pages are read where they lie
            host = [i for i, im in enumerate(self.images) if isinstance(im, np.ndarray) or not im.is_cuda]
            h_off = [0]
            for i in host:
                h, w, nc = self.geom[i][:3]
                h_off.append(h_off[-1] + _align(h * w * nc))
            src = [None] * n
            if host:
                stage = torch.empty(h_off[-1], dtype=torch.uint8).pin_memory()
                for k, i in enumerate(host):
                    im = self.images[i]
                    flat = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im.contiguous()
                    stage[h_off[k]:h_off[k] + flat.numel()].copy_(flat.reshape(-1))
                d_stage = stage.to(dev, non_blocking=True)
                for k, i in enumerate(host):
                    src[i] = d_stage[h_off[k]:]
            for i, im in enumerate(self.images):
                if src[i] is None:
                    src[i] = im.to(dev).contiguous()
            base = src[0].data_ptr()
            table = np.zeros((n, self._entry_width), np.int64)
            for i, g in enumerate(self.geom):
                self._table_entry(i, src[i].data_ptr() - base, g[1] * g[2], table[i])
            self._src = src                     # kept alive until collect
            d_tab = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
            self._ws = torch.empty(self.w_off[-1], dtype=torch.uint8, device=dev)
            self.out = torch.empty(self.o_off[-1], dtype=torch.uint8, device=dev)
            self.lengths = torch.empty(n, dtype=torch.int64, device=dev)
            self._tab, self._base = d_tab, base
            self.enqueue()
        return self

    def enqueue(self) -> None:
        """The launches alone, on the current stream (what tools/jpeg_encode_bench.py and tools/png_encode_bench.py time as "kernels")."""
        _lib.check(getattr(_lib.load(), self._c_encode_pages)(_dev_index(self.dev), self._base, self._tab.data_ptr(), len(self.images),
                                                              self.out.data_ptr(), self.lengths.data_ptr(), self._ws.data_ptr(),
                                                              self._ws.numel(), torch.cuda.current_stream(self.dev).cuda_stream))

    def _collect(self) -> List[bytes]:
        """Waits for the lengths, then copies the bytes the device wrote, and those alone, to the host."""
        n = len(self.images)
        if n == 0:
            return []
        lens = [int(v) for v in self.lengths.cpu()]
        for i, ln in enumerate(lens):
            if not 0 < ln <= self.caps[i]:
                raise RuntimeError(f"{self._name} encode: page {i} was skipped by the device (length {ln})")
        packed = torch.cat([self.out[self.o_off[i]:self.o_off[i] + lens[i]] for i in range(n)]) if n > 1 else self.out[:lens[0]]
        host = packed.cpu().numpy()
        ends = np.cumsum([0] + lens)
        return [host[ends[i]:ends[i + 1]].tobytes() for i in range(n)]


JPEG_SUBSAMPLINGS = {"4:2:0": 2, "4:4:4": 1}      # name -> luma sampling factor


def jpeg_quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """``ocrvi_jpeg_quant_tables`` (host only): the luminance and chrominance tables of ``quality``, uint16 [64] in natural order."""
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    _lib.check(_lib.load().ocrvi_jpeg_quant_tables(int(quality), luma.ctypes.data, chroma.ctypes.data))
    return luma, chroma


def jpeg_encode_header(height: int, width: int, components: int, subsampling: str = "4:2:0", quality: int = 95) -> bytes:
    """``ocrvi_jpeg_encode_header`` (host only): the bytes SOI .. SOS of the file ``imencode`` writes for such a page."""
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r}: expected one of {sorted(JPEG_SUBSAMPLINGS)}")
    buf = np.zeros(_lib.JPEG_HEADER_MAX, np.uint8)
    used = ctypes.c_size_t()
    _lib.check(_lib.load().ocrvi_jpeg_encode_header(int(width), int(height), int(components), JPEG_SUBSAMPLINGS[subsampling], int(quality),
                                                    buf.ctypes.data, buf.size, ctypes.byref(used)))
    return buf[:used.value].tobytes()


def jpeg_encode_sizes(height: int, width: int, components: int, subsampling: str = "4:2:0") -> dict:
    """``ocrvi_jpeg_encode_sizes`` (host only): ``blocks``, ``workspace_bytes``, ``scan_capacity`` and the workspace ``offsets`` of a page."""
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r}: expected one of {sorted(JPEG_SUBSAMPLINGS)}")
    blocks, wsb, cap = ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_uint64()
    offs = np.zeros(8, np.uint64)
    _lib.check(_lib.load().ocrvi_jpeg_encode_sizes(int(width), int(height), int(components), JPEG_SUBSAMPLINGS[subsampling], ctypes.byref(blocks),
                                                   ctypes.byref(wsb), ctypes.byref(cap), offs.ctypes.data))
    return {"blocks": blocks.value, "workspace_bytes": wsb.value, "scan_capacity": cap.value, "offsets": [int(v) for v in offs]}


class JpegEncodeJob(_EncodeJob):
    """The pages of one ``ocrvi_jpeg_encode_pages`` call (``_EncodeJob``): ``quality`` is a scalar or one value per page, ``geom`` holds
    (h, w, components, luma sampling factor) per page, ``collect_scans`` returns the entropy-coded scans and ``collect`` the files.
    ``imencode_pages`` is ``JpegEncodeJob(...).launch().collect()``."""
    _name, _entry_width, _c_encode_pages = "jpeg", _lib.JPEG_ENC_ENTRY, "ocrvi_jpeg_encode_pages"

    def __init__(self, images, quality=95, subsampling: str = "4:2:0", device="cuda:0", what: str = "imencode"):
        if subsampling not in JPEG_SUBSAMPLINGS:
            raise ValueError(f"{what}: subsampling {subsampling!r}: expected one of {sorted(JPEG_SUBSAMPLINGS)}")
        images = list(images)
        n = len(images)
        if isinstance(quality, (list, tuple, np.ndarray)):
            if len(quality) != n:
                raise ValueError(f"{what}: {len(quality)} qualities for {n} pages")
            qualities = list(quality)
        else:
            qualities = [quality] * n
        self.qualities = []
        for i, q in enumerate(qualities):
            if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= int(q) <= 100:
                raise ValueError(f"{what}: page {i}: quality {q!r} outside 1..100")
            self.qualities.append(int(q))
        self.subsampling = subsampling
        super().__init__(images, device, what)

    def _geom(self, h, w, nc):
        return h, w, nc, 1 if nc == 1 else JPEG_SUBSAMPLINGS[self.subsampling]

    def _sizes(self, i, h, w, nc):
        wsb, cap = ctypes.c_uint64(), ctypes.c_uint64()
        rc = _lib.load().ocrvi_jpeg_encode_sizes(w, h, nc, self.geom[i][3], None, ctypes.byref(wsb), ctypes.byref(cap), None)
        return rc, wsb.value, cap.value

    def _table_entry(self, i, src_offset, row_bytes, entry):
        h, w, nc, hs = self.geom[i]
        _lib.check(_lib.load().ocrvi_jpeg_encode_table_entry(w, h, nc, hs, self.qualities[i], src_offset, row_bytes, self.o_off[i], self.caps[i],
                                                             self.w_off[i], entry.ctypes.data))

    def collect_scans(self) -> List[bytes]:
        """Waits for the lengths, then copies the compressed bytes alone to the host."""
        return self._collect()

    def collect(self) -> List[bytes]:
        scans = self.collect_scans()
        return [jpeg_encode_header(h, w, nc, self.subsampling, self.qualities[i]) + scans[i] + b"\xff\xd9"
                for i, (h, w, nc, _) in enumerate(self.geom)]


def imencode_pages(images, quality=95, subsampling: str = "4:2:0", device: str = "cuda:0") -> List[bytes]:
    """``imencode`` for a list of pages of any sizes, grey and colour mixed, ``quality`` a scalar or one value per page: one upload of a
    page table and one set of launches (``ocrvi_jpeg_encode_pages``) serve the whole list; only the compressed bytes come back."""
    return JpegEncodeJob(images, quality, subsampling, device, "imencode_pages").launch().collect()


def imencode(image, quality: int = 95, subsampling: str = "4:2:0", device: str = "cuda:0") -> bytes:
    """``cv2.imencode(".jpg", image, [IMWRITE_JPEG_QUALITY, quality])`` for an RGB page: the bytes of a baseline JPEG file.  ``image`` is
    uint8 [h, w, 3] RGB or uint8 [h, w] grey (a one-component file), a numpy array or a tensor on the host or the device; ``subsampling`` is
    "4:2:0" (what cv2.imwrite and PIL write by default) or "4:4:4".  The host writes the header; everything else runs on the device.  The
    arithmetic is stated in include/ocrvi.h: libjpeg-turbo's default encoder byte for byte (PIL's ``save(..., "JPEG", quality=q)``), cv2
    parity unpinned.  ValueError for sides outside 1..65500, other dtypes, shapes or subsamplings, or a quality outside 1..100."""
    return JpegEncodeJob([image], quality, subsampling, device, "imencode").launch().collect()[0]


PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}      # name -> filter mode (OCRVI_PNG_FILTER_*)
PNG_ENC_REGIONS = ("filters", "stream", "hist", "lens", "cl_tokens", "records", "bit_offsets", "crc_partials", "info")


def png_encode_sizes(height: int, width: int, components: int) -> dict:
    """``ocrvi_png_encode_sizes`` (host only): ``stream_bytes``, ``blocks``, ``workspace_bytes``, ``out_capacity`` and the workspace
    ``offsets`` of a page."""
    stream, blocks, wsb, cap = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_uint64()
    offs = np.zeros(9, np.uint64)
    _lib.check(_lib.load().ocrvi_png_encode_sizes(int(width), int(height), int(components), ctypes.byref(stream), ctypes.byref(blocks),
                                                  ctypes.byref(wsb), ctypes.byref(cap), offs.ctypes.data))
    return {"stream_bytes": stream.value, "blocks": blocks.value, "workspace_bytes": wsb.value, "out_capacity": cap.value,
            "offsets": [int(v) for v in offs]}


class PngEncodeJob(_EncodeJob):
    """The pages of one ``ocrvi_png_encode_pages`` call (``_EncodeJob``): ``geom`` holds (h, w, components) and ``offsets`` the workspace
    regions per page, ``collect`` returns the files.  ``stage(i)`` reads page i's workspace regions for the tests.
    ``imencode_png_pages`` is ``PngEncodeJob(...).launch().collect()``."""
    _name, _entry_width, _c_encode_pages = "png", _lib.PNG_ENC_ENTRY, "ocrvi_png_encode_pages"

    def __init__(self, images, filters: str = "adaptive", device="cuda:0", what: str = "imencode_png"):
        if filters not in PNG_FILTERS:
            raise ValueError(f"{what}: filters {filters!r}: expected one of {sorted(PNG_FILTERS)}")
        self.filters = filters
        self.offsets = []
        super().__init__(images, device, what)

    def _sizes(self, i, h, w, nc):
        wsb, cap = ctypes.c_uint64(), ctypes.c_uint64()
        offs = np.zeros(9, np.uint64)
        rc = _lib.load().ocrvi_png_encode_sizes(w, h, nc, None, None, ctypes.byref(wsb), ctypes.byref(cap), offs.ctypes.data)
        if rc == 0:                             # offsets[i] belongs to page i: the base class calls this once per page, in page order
            self.offsets.append([int(v) for v in offs] + [wsb.value])
        return rc, wsb.value, cap.value

    def _table_entry(self, i, src_offset, row_bytes, entry):
        h, w, nc = self.geom[i]
        _lib.check(_lib.load().ocrvi_png_encode_table_entry(w, h, nc, PNG_FILTERS[self.filters], src_offset, row_bytes, self.o_off[i], self.caps[i],
                                                            self.w_off[i], entry.ctypes.data))

    def stage(self, i: int) -> dict:
        """Page i's workspace regions as uint8 arrays on the host, by the names of ``PNG_ENC_REGIONS`` (include/ocrvi.h states what each
        holds); for the tests."""
        o = self.offsets[i]
        ws = self._ws[self.w_off[i]:self.w_off[i] + o[9]].cpu().numpy()
        return {name: ws[o[k]:o[k + 1]] for k, name in enumerate(PNG_ENC_REGIONS)}

    def collect(self) -> List[bytes]:
        """Waits for the lengths, then copies the files' bytes alone to the host."""
        return self._collect()


def imencode_png_pages(images, filters: str = "adaptive", device: str = "cuda:0") -> List[bytes]:
    """``imencode_png`` for a list of pages of any sizes, grey and colour mixed: one upload of a page table and one set of launches
    (``ocrvi_png_encode_pages``) serve the whole list; only the files' bytes come back."""
    return PngEncodeJob(images, filters, device, "imencode_png_pages").launch().collect()


def imencode_png(image, filters: str = "adaptive", device: str = "cuda:0") -> bytes:
    """``cv2.imencode(".png", image)`` for an RGB page: the bytes of a PNG file (bit depth 8, colour type 2, or 0 for a grey page, no
    interlace, the chunks IHDR, one IDAT, IEND).  ``image`` is uint8 [h, w, 3] RGB or uint8 [h, w] grey, a numpy array or a tensor on the
    host or the device.  ``filters``: "adaptive" (libpng's heuristic per row) or one of "none", "sub", "up", "average", "paeth" for every
    row.  Filtering, deflate (distance-1 matches, the cheapest of stored, fixed and dynamic codes per 16 KiB block), both checksums and the
    file's assembly run on the device; the arithmetic is stated in include/ocrvi.h.  Lossless: ``imdecode`` (and zlib, PIL) read the pixels
    back exactly.  ValueError for other dtypes, shapes or filters, sides outside 1..65500, or a page whose IDAT could exceed 2^31 - 1 bytes."""
    return PngEncodeJob([image], filters, device, "imencode_png").launch().collect()[0]


IMWRITE_FORMATS = (None, "png")


def _check_format(format, what: str) -> None:
    if format not in IMWRITE_FORMATS:
        raise ValueError(f"{what}: format {format!r}: expected None (JPEG) or 'png'")


def imwrite(path: str, image, quality: int = 95, subsampling: str = "4:2:0", device: str = "cuda:0", format=None, filters: str = "adaptive") -> bool:
    """``cv2.imwrite(path, image)`` of the reference's loop (pipeline2.py:397-400) for an RGB page: ``imencode`` into the file -- JPEG
    whatever the suffix of ``path`` says -- or, with ``format="png"``, ``imencode_png`` (``quality`` and ``subsampling`` are then ignored).
    True when the file was written, False when it could not be (cv2's convention); ValueError as ``imencode`` / ``imencode_png``."""
    _check_format(format, "imwrite")
    data = imencode_png(image, filters, device) if format == "png" else imencode(image, quality, subsampling, device)
    try:
        with open(path, "wb") as f:
            f.write(data)
    except OSError:
        return False
    return True
