"""Generate the validation goldens in tests/golden/ by running the REFERENCE's own loss and validation modules.

Run only in the build container (needs the reference checkout, as make_golden.py does; only the .npz outputs travel):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py

model/det/loss.py, model/rec2/loss.py and src/det/val.py import with torch, numpy and tqdm alone and are loaded by path.
src/rec2/val.py needs `editdistance`, which is absent: its two functions (ten lines of arithmetic on strings) have no golden.

Fixtures (seeded inputs and the reference's outputs -- data only, no reference source):
  eval_det.npz : two batches of eight [2,1,32,48] maps; per batch the DBLoss dict and the compute_metrics dict, the k the reference
                 handed to torch.topk (captured from its own call), and validate_epoch's return over the two batches with a stub model
                 that returns the stored maps.  Batch 0 has more than three negatives per positive (k = 3 x positives) and a few
                 fractional gt / mask entries; batch 1 has fewer (k = every negative).
  eval_rec.npz : log_probs [24,6,232], targets, lengths; SVTRv2Loss (mean) and nn.CTCLoss(reduction='none') per sequence, with the
                 stored input lengths and with none.  Target lengths 0, 1, 5 (with an adjacent repeat), 8, 7 (input length 12 < T) and
                 10 on 6 steps (no alignment: +inf).
Two runs write the same bytes (one thread, fixed seeds, zip members dated 1980)."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
REF = "/root/reference"
sys.dont_write_bytecode = True
OUT = os.path.join(REPO, "tests", "golden")
N, H, W = 2, 32, 48
T, B, C = 24, 6, 232


def _load_ref(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def det_batch(seed, fill, fractional):
    """Eight seeded maps: gt = a few rectangles covering about `fill` of the page, logits that mostly agree with it."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((N, 1, H, W), np.float32)
    for n in range(N):
        while gt[n].mean() < fill:
            y, x = rng.integers(0, H - 6), rng.integers(0, W - 10)
            gt[n, 0, y:y + rng.integers(3, 7), x:x + rng.integers(5, 11)] = 1
    mask = np.ones_like(gt)
    mask[:, :, :, :3] = 0                                  # an ignored strip
    mask[0, 0, 10:13, 20:26] = 0                           # and an ignored box that cuts a text region or not
    logits = (rng.normal(0, 1.5, gt.shape) + (gt * 4 - 2)).astype(np.float32)
    tlogits = rng.normal(0, 1, gt.shape).astype(np.float32)
    if fractional:                                         # .byte() truncation and the == 1 / == 0 comparisons
        gt[0, 0, 5, 7:12] = [0.5, 0.25, 0.999, 0.75, 0.5]
        mask[1, 0, 20, 30:34] = [0.5, 0.999, 0.25, 0.75]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    binary = torch.sigmoid(t(logits))
    thresh = torch.sigmoid(t(tlogits))
    thresh_binary = torch.reciprocal(1 + torch.exp(-50 * (binary - thresh)))
    thresh_map = (0.3 + 0.4 * rng.random(gt.shape)).astype(np.float32)
    thresh_mask = (rng.random(gt.shape) < 0.35).astype(np.float32)
    pred = {"binary": binary, "thresh": thresh, "thresh_binary": thresh_binary, "bin_logits": t(logits), "thresh_logits": t(tlogits)}
    batch = {"gt": t(gt), "mask": t(mask), "thresh_map": t(thresh_map), "thresh_mask": t(thresh_mask)}
    return pred, batch


def det_golden():
    loss_mod = _load_ref("ref_det_loss", "model/det/loss.py")
    val_mod = _load_ref("ref_det_val", "src/det/val.py")
    criterion = loss_mod.DBLoss()
    preds, batches, out = [], [], {}
    topk_ks = []
    real_topk = torch.topk

    def spy_topk(x, k, *a, **kw):                          # the k the reference computed, from its own call
        topk_ks.append(int(k))
        return real_topk(x, k, *a, **kw)

    for i, (seed, fill, frac) in enumerate(((11, 0.10, True), (12, 0.45, False))):
        pred, batch = det_batch(seed, fill, frac)
        torch.topk = spy_topk
        try:
            with torch.no_grad():
                _, d = criterion(pred, batch)
        finally:
            torch.topk = real_topk
        m = val_mod.compute_metrics(pred["binary"], batch["gt"], batch["mask"])
        for k in ("binary", "thresh", "thresh_binary", "bin_logits"):
            out[f"b{i}_{k}"] = pred[k].numpy()
        for k, v in batch.items():
            out[f"b{i}_{k}"] = v.numpy()
        for k, v in d.items():
            out[f"b{i}_{k}"] = np.float64(v.item())
        for k, v in m.items():
            out[f"b{i}_{k}"] = np.float64(v)
        out[f"b{i}_k"] = np.int64(topk_ks[-1])
        print(f"eval_det batch {i}: k {topk_ks[-1]} loss {({k: float(v) for k, v in d.items()})} metrics {m}")
        batch = dict(batch, image=torch.full((N, 3, H, W), float(i)))
        preds.append(pred)
        batches.append(batch)

    class Stub(torch.nn.Module):                           # DBNetPP's call signature over the stored maps: the image carries its index
        def forward(self, images):
            return preds[int(images[0, 0, 0, 0])]

    avg_loss, avg = val_mod.validate_epoch(Stub(), batches, criterion, "cpu")
    out["val_loss"] = np.float64(avg_loss)
    for k, v in avg.items():
        out[f"val_{k}"] = np.float64(v)
    print(f"eval_det validate_epoch: loss {avg_loss} metrics {avg}")
    np.savez_compressed(os.path.join(OUT, "eval_det.npz"), **out)


def rec_golden():
    loss_mod = _load_ref("ref_rec_loss", "model/rec2/loss.py")
    g = torch.Generator().manual_seed(21)
    log_probs = torch.log_softmax(torch.randn(T, B, C, generator=g) * 3, dim=-1)
    rng = np.random.default_rng(22)
    lengths = [0, 1, 5, 8, 7, 10]
    input_lengths = [T, T, T, T, 12, 6]
    targets = np.ones((B, max(lengths)), np.int64)         # pad id 1
    for b, L in enumerate(lengths):
        targets[b, :L] = rng.integers(2, C, L)
    targets[2, 2] = targets[2, 1]                          # an adjacent repeat
    tg, tl, il = torch.from_numpy(targets), torch.tensor(lengths), torch.tensor(input_lengths)
    flat = torch.cat([tg[b, :L] for b, L in enumerate(lengths)])
    out = {"log_probs": log_probs.numpy(), "targets": targets.astype(np.int32), "target_lengths": np.array(lengths, np.int32),
           "input_lengths": np.array(input_lengths, np.int32)}
    with torch.no_grad():
        out["loss_mean"] = np.float64(loss_mod.SVTRv2Loss()(log_probs, tg, input_lengths=il, target_lengths=tl).item())
        out["loss_mean_default"] = np.float64(loss_mod.SVTRv2Loss()(log_probs, tg).item())
        none = torch.nn.CTCLoss(blank=0, reduction="none", zero_infinity=False)
        out["nll"] = none(log_probs, flat, il, tl).numpy().astype(np.float64)
        out["nll_full_length"] = none(log_probs, flat, torch.full((B,), T), tl).numpy().astype(np.float64)
    print(f"eval_rec: loss_mean {out['loss_mean']} default {out['loss_mean_default']} nll {out['nll']} full {out['nll_full_length']}")
    np.savez_compressed(os.path.join(OUT, "eval_rec.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(1)
    det_golden()
    rec_golden()
