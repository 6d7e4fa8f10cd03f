"""Validation on libocrvi -- the numbers the reference's two validation loops report, under the reference's names: ``DBLoss``
(model/det/loss.py:61-90), ``compute_metrics`` / ``validate_detection`` (src/det/val.py:13-118), ``SVTRv2Loss`` (model/rec2/loss.py:31-86,
CTC term), ``compute_cer`` / ``compute_acc`` / ``validate_recognition`` (src/rec2/val.py:14-87).

Forward values only: no backward pass and no SGM term (both are training).  Maps, log-probs and ids stay on the device; what comes back
per batch is ``ocrvi_det_eval``'s 104-byte record, ``nll [B]`` and ``dist [B]``.  The final divisions are host arithmetic on those."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .vocab import Tokenizer

_EPS = 1e-6   # loss.py:5,34,53 and val.py:38


def _device_of(*tensors, default="cuda:0") -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device(default)


def _dev_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _f32(t, device) -> torch.Tensor:
    return torch.as_tensor(t).to(device=device, dtype=torch.float32).contiguous()


def _i32(t, device) -> torch.Tensor:
    return torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()


def _id_rows(t, B: int, device) -> torch.Tensor:
    """int32 [B, L] on the device; an empty tensor becomes one column that no length reaches."""
    t = _i32(t, device)
    return t.reshape(B, t.numel() // B) if t.numel() else torch.full((B, 1), -1, dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------- detection
def _det_eval_workspace(N: int, H: int, W: int, dev: torch.device, have: Optional[torch.Tensor]) -> torch.Tensor:
    need = C.c_size_t()
    _lib.check(_lib.load().ocrvi_det_eval_workspace_bytes(N, H, W, C.byref(need)))
    if have is not None and have.numel() >= need.value and have.device == dev:
        return have
    return torch.empty(need.value, dtype=torch.uint8, device=dev)


def det_eval(binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask, negative_ratio: float = 3.0,
             workspace: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """``ocrvi_det_eval`` on eight (N,1,H,W) maps (host maps are copied to the device first): the record as a dict -- the six int64 counts
    ``tp, fp, fn, positive_count, negatives, negative_count`` and the seven float64 sums ``pos_bce, topk_bce, dice_inter, pred_mask, gt_mask,
    l1_num, thresh_mask`` (include/ocrvi.h).  Reading the record is the one synchronisation."""
    dev = _device_of(binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask)
    maps = [_f32(t, dev) for t in (binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask)]
    shape = tuple(maps[0].shape)
    if len(shape) != 4 or shape[1] != 1:
        raise ValueError(f"expected (N,1,H,W) maps, got {shape}")
    if any(tuple(m.shape) != shape for m in maps):
        raise ValueError(f"the eight maps differ in shape: {[tuple(m.shape) for m in maps]}")
    N, _, H, W = shape
    lib = _lib.load()
    workspace = _det_eval_workspace(N, H, W, dev, workspace)
    record = torch.empty(_lib.DET_EVAL_RECORD_BYTES // 8, dtype=torch.int64, device=dev)
    _lib.check(lib.ocrvi_det_eval(_dev_index(dev), *[m.data_ptr() for m in maps], N, H, W, float(negative_ratio), record.data_ptr(),
                                  workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(dev).cuda_stream))
    raw = record.cpu().numpy()
    ni = len(_lib.DET_EVAL_INT_SLOTS)
    out = {k: int(v) for k, v in zip(_lib.DET_EVAL_INT_SLOTS, raw[:ni])}
    out.update({k: float(v) for k, v in zip(_lib.DET_EVAL_F64_SLOTS, raw[ni:].view(np.float64))})
    return out


def db_loss_terms(rec: Dict[str, float], alpha: float = 5.0, beta: float = 10.0) -> Dict[str, float]:
    """The four numbers of DBLoss.forward's dict (loss.py:30,47-49,58,89) from a ``det_eval`` record, in float64."""
    l_prob = (rec["pos_bce"] + rec["topk_bce"]) / (rec["positive_count"] + rec["negative_count"] + _EPS)
    l_binary = 1.0 - 2.0 * rec["dice_inter"] / (rec["pred_mask"] + rec["gt_mask"] + _EPS)
    l_thresh = rec["l1_num"] / (rec["thresh_mask"] + _EPS)
    return {"loss": l_prob + alpha * l_binary + beta * l_thresh, "l_prob": l_prob, "l_binary": l_binary, "l_thresh": l_thresh}


def metrics_from_counts(tp: int, fp: int, fn: int) -> Dict[str, float]:
    """compute_metrics' ratios (src/det/val.py:38-51) from exact counts, in float32 and in the reference's order of operations."""
    f = np.float32
    tp, fp, fn, eps = f(tp), f(fp), f(fn), f(_EPS)
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    f1 = f(2) * precision * recall / (precision + recall + eps)
    iou = tp / (tp + fp + fn + eps)
    dice = f(2) * tp / (f(2) * tp + fp + fn + eps)
    return {"precision": float(precision), "recall": float(recall), "f1": float(f1), "iou": float(iou), "dice": float(dice)}


class DBLoss:
    """DBLoss(alpha, beta, ohem_ratio)(predictions, batch) -> (loss, {'loss','l_prob','l_binary','l_thresh'}) (model/det/loss.py:61-90):
    ``predictions`` is the dict ``DBNetPP.forward`` returns, ``batch`` has the reference dataloader's ``gt``, ``mask``, ``thresh_map`` and
    ``thresh_mask`` (host or device).  The values are 0-dim float64 tensors on the host; ``last_record`` keeps the record of the last
    call, which also holds the counts ``compute_metrics`` needs."""

    def __init__(self, alpha: float = 5.0, beta: float = 10.0, ohem_ratio: float = 3.0):
        self.alpha, self.beta, self.ohem_ratio = alpha, beta, ohem_ratio
        self.last_record: Optional[Dict[str, float]] = None
        self._ws: Optional[torch.Tensor] = None

    def forward(self, predictions, batch):
        dev = _device_of(predictions["binary"])
        N, _, H, W = predictions["binary"].shape
        self._ws = _det_eval_workspace(N, H, W, dev, self._ws)      # kept from batch to batch
        rec = det_eval(predictions["binary"], predictions["thresh"], predictions["thresh_binary"], predictions["bin_logits"],
                       batch["gt"], batch["mask"], batch["thresh_map"], batch["thresh_mask"], self.ohem_ratio, self._ws)
        self.last_record = rec
        terms = {k: torch.tensor(v, dtype=torch.float64) for k, v in db_loss_terms(rec, self.alpha, self.beta).items()}
        return terms["loss"], terms

    __call__ = forward


def compute_metrics(pred_binary, gt, mask, workspace: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Precision, recall, F1, IoU and dice of ``pred_binary > 0.5`` inside ``mask`` (src/det/val.py:13-51): the counts on the device, the
    ratios from the exact counts.

    Cost: this is a whole ``ocrvi_det_eval`` (all of its passes, for three of its counts) and, without ``workspace``, a fresh allocation
    of 4 bytes per pixel.  After ``DBLoss`` has run on the same batch its ``last_record`` already holds tp, fp and fn:
    ``metrics_from_counts`` on those costs nothing, and that is what ``validate_detection`` does.  Call this one for metrics without a
    loss, and pass the ``workspace`` of an earlier call (a uint8 device tensor of ``ocrvi_det_eval_workspace_bytes``) to keep it from
    allocating."""
    rec = det_eval(pred_binary, pred_binary, pred_binary, pred_binary, gt, mask, gt, mask, workspace=workspace)   # only tp, fp, fn are read
    return metrics_from_counts(rec["tp"], rec["fp"], rec["fn"])


def validate_detection(model, batches: Iterable[dict], criterion) -> Tuple[float, Dict[str, float]]:
    """validate_epoch of src/det/val.py:54-118 -> (avg_loss, metrics): the loss summed over the batches / their number, each metric the mean
    of the per-batch values.  ``model`` is a ``DBNetPP``; a batch has ``image``, ``gt``, ``mask``, ``thresh_map``, ``thresh_mask``."""
    total_loss, n_batches = 0.0, 0
    per_batch: Dict[str, List[float]] = {k: [] for k in ("precision", "recall", "f1", "iou", "dice")}
    for batch in batches:
        predictions = model(batch["image"])
        loss, _ = criterion(predictions, batch)
        total_loss += loss.item()          # (the record's copy synchronised the stream)
        if hasattr(model, "check_range"):
            model.check_range()
        rec = getattr(criterion, "last_record", None)
        metrics = metrics_from_counts(rec["tp"], rec["fp"], rec["fn"]) if rec is not None else \
            compute_metrics(predictions["binary"], batch["gt"], batch["mask"])
        for k in per_batch:
            per_batch[k].append(metrics[k])
        n_batches += 1
    if n_batches == 0:
        raise ValueError("validate_detection: no batches (the reference divides by len(dataloader))")
    return total_loss / n_batches, {k: float(np.mean(v)) for k, v in per_batch.items()}


# ---------------------------------------------------------------------------------------------- recognition
def ctc_nll(log_probs: torch.Tensor, targets, target_lengths, input_lengths=None, blank: int = 0) -> torch.Tensor:
    """``ocrvi_ctc_loss``: (T,B,C) float32 log-probs on the device, (B,L) targets -> nll float64 [B] on the device (+inf where no alignment
    exists)."""
    if not (isinstance(log_probs, torch.Tensor) and log_probs.is_cuda):
        raise ValueError("log_probs must be a device tensor (what SVTRv2.forward returns)")
    dev = log_probs.device
    lp = log_probs.to(dtype=torch.float32).contiguous()
    T, B, Cn = lp.shape
    tg = _id_rows(targets, B, dev)
    tl = _i32(target_lengths, dev).reshape(B)
    il = None if input_lengths is None else _i32(input_lengths, dev).reshape(B)
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().ocrvi_ctc_loss(_dev_index(dev), lp.data_ptr(), T, B, Cn, tg.data_ptr(), tg.shape[1], tl.data_ptr(), _lib.ptr(il),
                                          blank, nll.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return nll


class SVTRv2Loss:
    """SVTRv2Loss(blank, pad_id, ...)(log_probs, targets, sgm_output=None, input_lengths=None, target_lengths=None)
    (model/rec2/loss.py:31-86), the CTC term: nn.CTCLoss(blank, reduction, zero_infinity) of (T,B,C) device log-probs.  Returns a float64
    tensor on the host (0-dim for 'mean' and 'sum').  The SGM term is training only: ``sgm_output`` must be None."""

    def __init__(self, blank: int = 0, pad_id: int = 1, lambda_sgm: float = 0.1, reduction: str = "mean", zero_infinity: bool = True):
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.blank, self.pad_id, self.lambda_sgm, self.reduction, self.zero_infinity = blank, pad_id, lambda_sgm, reduction, zero_infinity

    def forward(self, log_probs, targets, sgm_output=None, input_lengths=None, target_lengths=None):
        if sgm_output is not None:
            raise NotImplementedError("the SGM loss terms (loss.py:66-82) are training only; validation passes sgm_output=None")
        targets = torch.as_tensor(targets)
        if target_lengths is None:
            target_lengths = (targets != self.pad_id).sum(dim=1)      # loss.py:51
        lengths = torch.as_tensor(target_lengths).reshape(-1).cpu().to(torch.float64)
        nll = ctc_nll(log_probs, targets, target_lengths, input_lengths, self.blank).cpu()
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "mean":       # nn.CTCLoss: each loss over its target length (at least 1), then the mean over the batch
            return (nll / lengths.clamp_min(1)).mean()
        return nll.sum() if self.reduction == "sum" else nll

    __call__ = forward


def edit_distance_ids(pred_ids, pred_lens, gt_ids, gt_lens) -> torch.Tensor:
    """``ocrvi_edit_distance``: int32 id rows (B,T) / (B,G) with their lengths -> dist int32 [B] on the device.  Ids < 2 of the prediction
    rows are dropped first (blank and pad, tokenizer.py:73)."""
    dev = _device_of(pred_ids, gt_ids)
    pl, gl = _i32(pred_lens, dev), _i32(gt_lens, dev)
    B = pl.numel()
    p, g = _id_rows(pred_ids, B, dev), _id_rows(gt_ids, B, dev)
    dist = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ocrvi_edit_distance(_dev_index(dev), p.data_ptr(), p.shape[1], pl.data_ptr(), g.data_ptr(), g.shape[1],
                                               gl.data_ptr(), B, dist.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream))
    return dist


def _rows(seqs: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    lens = np.array([len(s) for s in seqs], np.int32)
    rows = np.full((len(seqs), max(1, int(lens.max()) if len(seqs) else 1)), -1, np.int32)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = s
    return rows, lens


def encode_ground_truth(texts: Sequence[str], tokenizer: Tokenizer) -> Tuple[np.ndarray, np.ndarray]:
    """Ground-truth strings -> (ids int32 [B,G], lens int32 [B]) for ``edit_distance_ids``: one id per character, -2 for a character
    outside the alphabet (it equals no prediction id, as in the string distance)."""
    return _rows([[tokenizer.token_to_id.get(c, -2) for c in t] for t in texts])


def _string_distances(predictions: Sequence[str], ground_truths: Sequence[str], device="cuda:0") -> List[int]:
    pairs = list(zip(predictions, ground_truths))
    if not pairs:
        return []
    local = {c: i + 2 for i, c in enumerate(sorted({c for p, g in pairs for c in p + g}))}   # exact for any two strings
    p, pl = _rows([[local[c] for c in a] for a, _ in pairs])
    g, gl = _rows([[local[c] for c in b] for _, b in pairs])
    dev = torch.device(device)
    return edit_distance_ids(torch.from_numpy(p).to(dev), torch.from_numpy(pl).to(dev), torch.from_numpy(g).to(dev),
                             torch.from_numpy(gl).to(dev)).cpu().tolist()


def compute_cer(predictions: List[str], ground_truths: List[str]) -> float:
    """Character error rate (src/rec2/val.py:14-24): summed edit distances over summed ground-truth lengths (at least 1)."""
    pairs = list(zip(predictions, ground_truths))
    errors = sum(_string_distances(predictions, ground_truths))
    return errors / max(sum(len(g) for _, g in pairs), 1)


def compute_acc(predictions: List[str], ground_truths: List[str]) -> float:
    """Exact-match accuracy (src/rec2/val.py:27-30)."""
    return sum(1 for p, g in zip(predictions, ground_truths) if p == g) / max(len(predictions), 1)


def greedy_ids(log_probs: torch.Tensor, blank: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ocrvi_ctc_greedy`` on (T,B,C) device log-probs -> (ids int32 [B,T], lens int32 [B]) on the device: the collapsed greedy path that
    ``SVTRv2.decode_probs`` turns into strings."""
    lp = log_probs.to(dtype=torch.float32).contiguous()
    T, B, Cn = lp.shape
    am = torch.empty((B, T), dtype=torch.int32, device=lp.device)
    ids, lens = torch.empty_like(am), torch.empty(B, dtype=torch.int32, device=lp.device)
    _lib.check(_lib.load().ocrvi_ctc_greedy(_dev_index(lp.device), lp.data_ptr(), T, B, Cn, blank, am.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                            torch.cuda.current_stream(lp.device).cuda_stream))
    return ids, lens


def validate_recognition(model, batches: Iterable[dict], criterion) -> Tuple[float, Dict[str, float]]:
    """validate_epoch of src/rec2/val.py:33-87 -> (avg_loss, {'cer', 'accuracy'}): the loss summed over the batches / their number, CER and
    accuracy pooled over all samples.  ``model`` is an ``SVTRv2``; a batch has ``image``, ``target``, ``target_length``, ``text`` and
    optionally ``input_length``.  The greedy path is decoded and compared with the encoded ground truth on the device (no strings are
    formed): a prediction equals its ground truth exactly when their distance is 0."""
    total_loss, n_batches = 0.0, 0
    errors = chars = correct = samples = 0
    for batch in batches:
        log_probs = model(batch["image"])
        loss = criterion(log_probs, batch["target"], input_lengths=batch.get("input_length"), target_lengths=batch["target_length"])
        total_loss += loss.item()
        ids, lens = greedy_ids(log_probs, model.blank_id)
        texts = list(batch["text"])
        gt, gt_lens = encode_ground_truth(texts, model.tokenizer)
        dist = edit_distance_ids(ids, lens, torch.from_numpy(gt).to(ids.device), torch.from_numpy(gt_lens).to(ids.device)).cpu().tolist()
        if hasattr(model, "check_range"):
            model.check_range()            # (the copy above synchronised the stream)
        errors += sum(dist)
        correct += sum(1 for d in dist if d == 0)
        chars += sum(len(t) for t in texts)
        samples += len(texts)
        n_batches += 1
    return total_loss / max(n_batches, 1), {"cer": errors / max(chars, 1), "accuracy": correct / max(samples, 1)}
