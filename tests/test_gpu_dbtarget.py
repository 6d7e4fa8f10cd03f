"""``DetectionDataset`` and its two kernels (``ocrvi_db_target_maps``, ``ocrvi_resize_normalize_pad_pages``) on the device against the
Python statement of the reference's dataloader in tests/dbtarget_ref.py: every tensor BIT-EQUAL.  The reference is computed once per
(image, S) and shared."""
import json
import math
import os

import numpy as np
import pytest
import torch

import dbtarget_ref as R
from oracle.dbpost_cpu import polygon_mask
from ocr_vi_invoice_amd import _lib, data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("image", "gt", "mask", "thresh_map", "thresh_mask")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")

SQUARE = [(0, 0), (100, 0), (100, 100), (0, 100)]
STRIP = [(0, 0), (100, 0), (100, 6), (0, 6)]
DUMBBELL = [(0, 0), (40, 0), (40, 18), (60, 18), (60, 0), (100, 0), (100, 40), (60, 40), (60, 22), (40, 22), (40, 40), (0, 40)]


def _shift(p, dx, dy, s=1.0):
    return [(x * s + dx, y * s + dy) for x, y in p]


def _comb(x0, y0, teeth, tooth_w, gap, height, base):
    """`teeth` teeth: a row through them crosses 2 * teeth edges"""
    pts = [(x0, y0 + height + base), (x0, y0)]
    x = x0
    for t in range(teeth):
        pts += [(x + tooth_w, y0), (x + tooth_w, y0 + height)]
        x += tooth_w + gap
        if t + 1 < teeth:
            pts += [(x, y0 + height), (x, y0)]
    pts += [(x - gap, y0 + height + base)]
    return pts


def _circle(cx, cy, r, n):
    return [(cx + r * math.cos(2 * math.pi * k / n), cy + r * math.sin(2 * math.pi * k / n)) for k in range(n)]


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# h x w: 61 x 97 and 200 x 120 scale down (pad below / right), 64 x 40 is scale 1.0 at S = 64 and scales up at 96, 30 x 50 scales up
SAMPLES = [
    (_image(61, 97, 1), [_comb(4, 6, 12, 3, 4, 30, 8),                       # 24 crossings per row
                         [(70, 2), (94, 58), (70, 2.05)],                    # a steep sliver of area 0.6: the ignore fill is its boundary line alone
                         [(50, 2), (53, 2), (68, 58)],                       # a steep thin triangle: boundary pixels beside every span
                         _shift(SQUARE, 60, 35, 0.3), [(0, 40), (10, 50), (10, 40), (0, 50)]]),
    (_image(64, 40, 2), [_shift(DUMBBELL, 2, 4, 0.36), [(5, 30), (38, 28), (45, 70), (3, 60)],   # the second one leaves the image
                         [(10, 22), (30, 22.4), (10, 22.8)], _circle(20, 45, 9.5, 40)]),
    (_image(30, 50, 3), [[(2, 2), (20, 3), (22, 12), (4, 11)], [(30, 5), (48, 5), (48, 28), (30, 28)], [(25, 20), (28, 20), (28, 22), (25, 22)]]),
    (_image(200, 120, 4), [SQUARE, _shift(STRIP, 5, 102), _shift(DUMBBELL, 10, 110), [(0, 160), (10, 170), (10, 160), (0, 170)], [(0, 180), (50, 180), (50, 180.01)],
                           [(90, 150), (150, 150), (150, 199), (90, 199)], [(20, 190), (50, 190), (50, 192), (20, 192)],
                           _circle(60, 60, 55.5, 300)]),
    (_image(45, 45, 5), []),                                                  # no polygon at all
]
_REFS = {}


def ref(i, S, thresh=True):
    if (i, S, thresh) not in _REFS:
        img, polys = SAMPLES[i]
        _REFS[(i, S, thresh)] = R.load_sample(img, polys, S, 0.4, 0.7, thresh)
    return _REFS[(i, S, thresh)]


def equal(got, want, what):
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, (what, k, g.shape)
        bad = np.argwhere(g.view(np.uint32) != want[k].view(np.uint32))
        assert len(bad) == 0, f"{what} {k}: {len(bad)} elements differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


@pytest.fixture(scope="module", params=[64, 96])
def batch(request):
    S = request.param
    ds = data.DetectionDataset(samples=SAMPLES, image_size=S, thresh_maps=True, device=DEV)
    out = list(ds.batches(8))
    assert len(out) == 1 and len(ds) == 5 and ds.blank == []
    return S, ds, out[0]


def test_batch_of_mixed_sizes_equals_the_reference(batch):
    S, _, out = batch
    for i in range(len(SAMPLES)):
        r = ref(i, S)
        assert r["gt"].any() or i == 4
        equal({k: out[k][i] for k in KEYS}, r, f"S={S} sample {i}")
    assert all(out[k].shape == (5, 3 if k == "image" else 1, S, S) and out[k].is_cuda for k in KEYS)


def test_the_cases_hold_what_they_claim(batch):
    S, _, _ = batch
    assert R.resize_sizes(64, 40, 64)[0] == 1.0 and R.resize_sizes(61, 97, 64)[0] < 1 and R.resize_sizes(30, 50, 64)[0] > 1
    kinds = [[k for k, _ in R.polygon_jobs(img.shape[0], img.shape[1], polys, 0.4, True)] for img, polys in SAMPLES]
    assert all({R.GT, R.MASK, R.THRESH} <= set(k) for k in kinds[:4]) and kinds[4] == []
    comb = [(int(x), int(y)) for x, y in SAMPLES[0][1][0]]
    assert sum(1 for a, b in zip(comb, comb[1:] + comb[:1]) if (a[1] <= 20 < b[1]) or (b[1] <= 20 < a[1])) > 16
    sliver = np.array(SAMPLES[0][1][1], np.int64)
    n_fill = int(polygon_mask(sliver, 61, 97).sum())
    assert n_fill == 57 and R.polygon_jobs(61, 97, [SAMPLES[0][1][1]])[0][0] == R.MASK     # a pixel per row: the line, no span at all
    out_of_image = [p for k, p in R.polygon_jobs(64, 40, SAMPLES[1][1], 0.4, True) if k == R.THRESH]
    assert any(min(x for x, _ in p) < 0 or max(x for x, _ in p) > 39 or max(y for _, y in p) > 63 for p in out_of_image)
    r = ref(3, S)
    assert (r["thresh_map"][r["thresh_mask"] == 1] == np.float32(0.7)).all() and (r["mask"] == 0).any() and (r["thresh_mask"] == 1).any()


def test_each_image_alone_and_getitem_equal_the_batch_row(batch):
    S, ds, out = batch
    for i in range(len(SAMPLES)):
        one = ds[i]
        alone = next(data.DetectionDataset(samples=[SAMPLES[i]], image_size=S, thresh_maps=True, device=DEV).batches(1))
        for k in KEYS:
            assert one[k].shape == out[k].shape[1:] and torch.equal(one[k], out[k][i]), (i, k)
            assert torch.equal(alone[k][0], out[k][i]), (i, k)
    parts = list(ds.batches(2))
    assert [p["gt"].shape[0] for p in parts] == [2, 2, 1]
    assert all(torch.equal(torch.cat([p[k] for p in parts]), out[k]) for k in KEYS)


def test_without_thresh_maps_the_threshold_maps_stay_zero():
    ds = data.DetectionDataset(samples=SAMPLES[:4], image_size=64, device=DEV)
    out = next(ds.batches(4))
    for i in range(4):
        equal({k: out[k][i] for k in KEYS}, ref(i, 64, False), f"sample {i}")
    assert not out["thresh_map"].any() and not out["thresh_mask"].any()


def _maps(jobs, points, rows, S, thresh_max=0.7):
    n = len(rows)
    j = torch.tensor(np.asarray(jobs, np.int32).reshape(-1, 8), device=DEV)
    p = torch.tensor(np.asarray(points, np.int32).reshape(-1, 2), device=DEV)
    r = torch.tensor(np.asarray(rows, np.int32).reshape(-1, 4), device=DEV)
    out = [torch.full((n, 1, S, S), 9.0, device=DEV) for _ in range(4)]
    _lib.check(_lib.load().ocrvi_db_target_maps(0, j.data_ptr(), len(j), p.data_ptr(), len(p), r.data_ptr(), n, S, thresh_max,
                                                *[o.data_ptr() for o in out], torch.cuda.current_stream().cuda_stream))
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("S", [63, 96])          # 63: the scalar stores of the init kernel
def test_a_polygon_longer_than_the_lds_stage_and_jobs_out_of_bounds(S):
    h, w = 90, 130
    rng = np.random.default_rng(7)
    ang = np.sort(rng.uniform(0, 2 * math.pi, 2500))
    star = np.stack([65 + rng.uniform(20, 80, 2500) * np.cos(ang), 45 + rng.uniform(20, 60, 2500) * np.sin(ang)], 1).astype(np.int32)   # leaves the image
    tri = np.array([(5, 5), (40, 8), (20, 30)], np.int32)
    pts = np.concatenate([star, tri])
    box = lambda q: [int(q[:, 0].min()), int(q[:, 1].min()), int(q[:, 0].max()), int(q[:, 1].max())]
    jobs = [[0, R.GT, 0, 2500] + box(star), [0, R.THRESH, 2500, 2503] + box(tri),
            [1, R.MASK, 2500, 2503] + box(tri),                       # image 1 is a blank row: nothing may be written for it
            [2, R.GT, 0, 3] + box(tri), [0, R.GT, 2500, 2504] + box(tri), [0, 3, 0, 3] + box(tri), [0, R.MASK, -1, 3] + box(tri)]   # all skipped
    _, nh, nw = R.resize_sizes(h, w, S)
    gt, mask, tmap, tmask = _maps(jobs, pts, [[h, w, nh, nw], [h, w, 0, 0]], S)
    want = np.zeros((S, S), np.float32)
    want[:nh, :nw] = R.nearest_resize(polygon_mask(star, h, w).astype(np.float32), nw, nh)
    assert want.any() and not want[:nh, :nw].all() and (gt[0, 0] == want).all()
    wt = np.zeros((S, S), np.float32)
    wt[:nh, :nw] = R.nearest_resize(polygon_mask(tri, h, w).astype(np.float32), nw, nh)
    assert (tmask[0, 0] == wt).all() and (tmap[0, 0] == wt * np.float32(0.7)).all()
    inside = np.zeros((S, S), np.float32)
    inside[:nh, :nw] = 1
    assert (mask[0, 0] == inside).all()
    assert not gt[1].any() and not mask[1].any() and not tmap[1].any() and not tmask[1].any()


def test_jpeg_sample_equals_its_decoded_array():
    z = np.load(GOLD)
    name = "s97x131_420_q85"
    polys = [[(10, 10), (90, 12), (88, 50), (12, 48)], [(100, 60), (125, 60), (125, 90), (100, 90)]]
    a = next(data.DetectionDataset(samples=[(z["j_" + name].tobytes(), polys)], image_size=64, thresh_maps=True, device=DEV).batches(1))
    b = next(data.DetectionDataset(samples=[(z["p_" + name], polys)], image_size=64, thresh_maps=True, device=DEV).batches(1))
    c = next(data.DetectionDataset(samples=[(torch.from_numpy(z["p_" + name]).to(DEV), polys)], image_size=64, thresh_maps=True, device=DEV).batches(1))
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in KEYS)
    equal({k: a[k][0] for k in KEYS}, R.load_sample(z["p_" + name], polys, 64, 0.4, 0.7, True), name)


def test_data_dir_blank_samples_and_files_the_library_cannot_read(tmp_path):
    z = np.load(GOLD)
    name = "s97x131_420_q85"
    polys = [[[10, 10], [90, 12], [88, 50], [12, 48]], [[1, 1], [2, 2]]]            # the second has fewer than 3 points: dropped
    ann = {"annotations": [{"polygon": p, "text": "x"} for p in polys]}
    (tmp_path / "a.json").write_text(json.dumps(ann))
    (tmp_path / "a.jpg").write_bytes(z["j_" + name].tobytes())
    (tmp_path / "b.json").write_text(json.dumps(ann))                                # no image beside it
    (tmp_path / "c.json").write_text("{ not json")
    (tmp_path / "c.jpg").write_bytes(z["j_" + name].tobytes())
    (tmp_path / "d.json").write_text(json.dumps({"annotations": [{"text": "no polygon key"}]}))
    (tmp_path / "d.jpg").write_bytes(z["j_" + name].tobytes())
    ds = data.DetectionDataset(str(tmp_path), image_size=64, device=DEV)
    assert len(ds) == 4
    out = next(ds.batches(4))
    equal({k: out[k][0] for k in KEYS}, R.load_sample(z["p_" + name], polys[:1], 64), "a")
    blank = R.blank_sample(64)
    for i in (1, 2, 3):
        equal({k: out[k][i] for k in KEYS}, blank, f"blank {i}")
    assert [i for i, _ in ds.blank] == [1, 2, 3] and "Cannot read image" in ds.blank[0][1]
    ds[1]
    assert len(ds.blank) == 3                                                        # recorded once
    # a side that resizes to 0: 1 x 200 at S = 64 -> int(1 * 0.32) = 0
    thin = data.DetectionDataset(samples=[(np.zeros((1, 200, 3), np.uint8), []), SAMPLES[2]], image_size=64, device=DEV)
    out = next(thin.batches(2))
    equal({k: out[k][0] for k in KEYS}, blank, "thin")
    equal({k: out[k][1] for k in KEYS}, ref(2, 64, False), "beside a blank one")
    assert thin.blank == [(0, "1 x 200 resizes to 0 x 64")]
    # what cv2 would read and the library cannot must not be blanked
    for sub, fname, payload, word in (("png", "e.png", b"\x89PNG\r\n\x1a\n" + bytes(32), "e.png"),
                                      ("prog", "e.jpg", z["j_progressive_33x17"].tobytes(), "e.jpg")):
        d = tmp_path / sub
        d.mkdir()
        (d / "e.json").write_text(json.dumps(ann))
        (d / fname).write_bytes(payload)
        bad = data.DetectionDataset(str(d), image_size=64, device=DEV)
        with pytest.raises(ValueError, match=word):
            bad[0]
        assert bad.blank == []


def test_validate_detection_on_the_dataset_equals_reference_batches():
    from ocr_vi_invoice_amd import DBNetPP, weights
    from ocr_vi_invoice_amd.val import DBLoss, validate_detection
    model = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=5), dtype="f32", device=DEV)
    ds = data.DetectionDataset(samples=SAMPLES[:4], image_size=64, thresh_maps=True, device=DEV)
    got = validate_detection(model, ds.batches(2), DBLoss())
    ref_batches = [{k: torch.from_numpy(np.stack([ref(i, 64)[k] for i in pair])).to(DEV) for k in KEYS} for pair in ((0, 1), (2, 3))]
    want = validate_detection(model, ref_batches, DBLoss())
    assert got == want and math.isfinite(got[0]) and set(got[1]) == {"precision", "recall", "f1", "iou", "dice"}
