"""numpy int64 restatement of the enhance_document arithmetic that include/ocrvi.h defines (src/preprocess/scanner.py:55-76: Lab, CLAHE on
L, non-local means, sharpen).  Pages are RGB uint8 HWC.  The tables are built in float64 and rounded with rint, as the library's host code
does; every stage after that is integer, so the device must agree bit for bit.  Parity with cv2 itself is unpinned (cv2 is not available)."""
import numpy as np

M = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]]
TABLE_ORDER = (("LIN", 256), ("F", 2041), ("ENC", 2041), ("FY", 256), ("DA", 256), ("DB", 256), ("W1", 1024), ("W2", 1024), ("CF", 9), ("CI", 9))


def _fix_rows(a):
    a = np.asarray(a, np.int64).reshape(3, 3).copy()
    for r in a:
        r[int(np.argmax(np.abs(r)))] += 4096 - int(r.sum())
    return a


def _build():
    v = np.arange(256, dtype=np.float64)
    c = v / 255.0
    t = {}
    t["LIN"] = np.rint(2040.0 * np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4))
    x = np.arange(2041, dtype=np.float64) / 2040.0
    t["F"] = np.rint(32768.0 * np.where(x > 216.0 / 24389.0, np.cbrt(x), (841.0 / 108.0) * x + 4.0 / 29.0))
    t["ENC"] = np.rint(255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055))
    t["FY"] = np.rint((v * 100.0 / 255.0 + 16.0) / 116.0 * 32768.0)
    t["DA"] = np.rint((v - 128.0) * 32768.0 / 500.0)
    t["DB"] = np.rint((v - 128.0) * 32768.0 / 200.0)
    d = np.arange(1024, dtype=np.float64) * 64.0 / 49.0
    t["W1"] = np.rint(255.0 * np.exp(-d / 100.0))
    t["W2"] = np.rint(255.0 * np.exp(-d / 200.0))
    m = M
    white = [m[i][0] + m[i][1] + m[i][2] for i in range(3)]
    c00, c01, c02 = m[1][1] * m[2][2] - m[1][2] * m[2][1], m[1][2] * m[2][0] - m[1][0] * m[2][2], m[1][0] * m[2][1] - m[1][1] * m[2][0]
    det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02
    adj = [[c00, m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]],
           [c01, m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]],
           [c02, m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]]]
    t["CF"] = _fix_rows([[np.rint(4096.0 * m[i][j] / white[i]) for j in range(3)] for i in range(3)])
    t["CI"] = _fix_rows([[np.rint(4096.0 * (adj[i][j] / det) * white[j]) for j in range(3)] for i in range(3)])
    return {k: np.asarray(a).astype(np.int64) for k, a in t.items()}


T = _build()


def tables_blob() -> bytes:
    """The tables as ``ocrvi_enhance_tables`` lays them out: int32 each, in TABLE_ORDER."""
    return b"".join(T[k].astype(np.int32).reshape(-1).tobytes() for k, _ in TABLE_ORDER)


def rgb_to_lab(rgb):
    lin = T["LIN"][np.asarray(rgb, np.int64)]
    xyz = (lin @ T["CF"].T + 2048) >> 12
    f = T["F"][xyz]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    L = np.clip((2958 * fy - 13369344 + 163840) // 327680, 0, 255)
    a = np.clip(((500 * (fx - fy) + 16384) >> 15) + 128, 0, 255)
    b = np.clip(((200 * (fy - fz) + 16384) >> 15) + 128, 0, 255)
    return np.stack([L, a, b], -1).astype(np.uint8)


def _lab_t(f):
    hi = (f ** 3 * 2040 + (1 << 44)) >> 45
    lo = np.maximum(((f - 4520) * 8383 + (1 << 19)) >> 20, 0)
    return np.where(f > 6781, hi, lo)


def lab_to_rgb(lab):
    lab = np.asarray(lab, np.int64)
    fy = T["FY"][lab[..., 0]]
    fx = np.clip(fy + T["DA"][lab[..., 1]], 0, 49151)
    fz = np.clip(fy - T["DB"][lab[..., 2]], 0, 49151)
    t = np.stack([_lab_t(fx), _lab_t(np.clip(fy, 0, 49151)), _lab_t(fz)], -1)
    r = np.clip((t @ T["CI"].T + 2048) >> 12, 0, 2040)
    return T["ENC"][r].astype(np.uint8)


def clahe_luts(plane):
    """(LUTs int64 [8, 8, 256], th, tw) of a uint8 plane."""
    plane = np.asarray(plane, np.int64)
    H, W = plane.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    p = np.pad(plane, ((0, Hp - H), (0, Wp - W)), mode="reflect")
    th, tw = Hp // 8, Wp // 8
    area = th * tw
    clip = max(2 * area // 256, 1)
    luts = np.zeros((8, 8, 256), np.int64)
    for ty in range(8):
        for tx in range(8):
            hist = np.bincount(p[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].reshape(-1), minlength=256).astype(np.int64)
            excess = int(np.maximum(hist - clip, 0).sum())
            hist = np.minimum(hist, clip) + excess // 256
            r = excess % 256
            if r > 0:
                step = max(256 // r, 1)
                hist[np.arange(r) * step] += 1
            luts[ty, tx] = (255 * np.cumsum(hist) + area // 2) // area
    return luts, th, tw


def clahe_plane(plane):
    plane = np.asarray(plane, np.int64)
    H, W = plane.shape
    luts, th, tw = clahe_luts(plane)
    nx, ny = 2 * np.arange(W) + 1 - tw, 2 * np.arange(H) + 1 - th
    tx1, ty1 = nx // (2 * tw), ny // (2 * th)
    ax, ay = (nx - tx1 * 2 * tw)[None, :], (ny - ty1 * 2 * th)[:, None]
    tx2, ty2 = np.clip(tx1 + 1, 0, 7)[None, :], np.clip(ty1 + 1, 0, 7)[:, None]
    tx1, ty1 = np.clip(tx1, 0, 7)[None, :], np.clip(ty1, 0, 7)[:, None]
    bx, by = 2 * tw - ax, 2 * th - ay
    s = bx * by * luts[ty1, tx1, plane] + ax * by * luts[ty1, tx2, plane] + bx * ay * luts[ty2, tx1, plane] + ax * ay * luts[ty2, tx2, plane]
    return ((s + 2 * tw * th) // (4 * tw * th)).astype(np.uint8)


def clahe_lab(lab):
    out = np.array(lab, np.uint8)
    out[..., 0] = clahe_plane(out[..., 0])
    return out


def nlm_planes(planes, wtab, stats=None):
    """NLM (template 7, search 21) of the [H, W, C] group ``planes`` under the weight table ``wtab``; box sums by cumulative sums.
    ``stats``: a dict that receives the mean number of non-centre offsets with a non-zero weight per pixel."""
    I = np.asarray(planes, np.int64)
    H, W, C = I.shape
    P = np.pad(I, ((13, 13), (13, 13), (0, 0)), mode="reflect")
    A = P[10:H + 16, 10:W + 16]
    acc, sw, live = np.zeros((H, W, C), np.int64), np.zeros((H, W), np.int64), 0
    for dy in range(-10, 11):
        for dx in range(-10, 11):
            sq = ((A - P[10 + dy:H + 16 + dy, 10 + dx:W + 16 + dx]) ** 2).sum(-1)
            S = np.zeros((H + 7, W + 7), np.int64)
            S[1:, 1:] = sq.cumsum(0).cumsum(1)
            D = S[7:, 7:] - S[:-7, 7:] - S[7:, :-7] + S[:-7, :-7]
            w = wtab[np.minimum(D >> 6, 1023)]
            acc += w[..., None] * P[13 + dy:13 + dy + H, 13 + dx:13 + dx + W]
            sw += w
            if dy or dx:
                live += int((w > 0).sum())
    if stats is not None:
        stats["live_offsets"] = live / (H * W)
    return ((acc + (sw // 2)[..., None]) // sw[..., None]).astype(np.uint8)


def nlm_planes_direct(planes, wtab):
    """The same by the definition: a 7 x 7 loop per pixel and offset (small planes only)."""
    I = np.asarray(planes, np.int64)
    H, W, C = I.shape
    P = np.pad(I, ((13, 13), (13, 13), (0, 0)), mode="reflect")
    out = np.zeros((H, W, C), np.uint8)
    for y in range(H):
        for x in range(W):
            a = P[y + 10:y + 17, x + 10:x + 17]
            acc, sw = np.zeros(C, np.int64), 0
            for dy in range(-10, 11):
                for dx in range(-10, 11):
                    D = int(((a - P[y + 10 + dy:y + 17 + dy, x + 10 + dx:x + 17 + dx]) ** 2).sum())
                    w = int(wtab[min(D >> 6, 1023)])
                    acc += w * P[y + 13 + dy, x + 13 + dx]
                    sw += w
            out[y, x] = (acc + sw // 2) // sw
    return out


def nlm_lab(lab, stats=None):
    lab = np.asarray(lab, np.uint8)
    s1, s2 = {}, {}
    out = np.concatenate([nlm_planes(lab[..., :1], T["W1"], s1), nlm_planes(lab[..., 1:], T["W2"], s2)], -1)
    if stats is not None:
        stats["L"], stats["ab"] = s1["live_offsets"], s2["live_offsets"]
    return out


def sharpen(img):
    p = np.pad(np.asarray(img, np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    H, W = img.shape[:2]
    s = sum(p[j:j + H, i:i + W] for j in range(3) for i in range(3))
    return np.clip(10 * p[1:-1, 1:-1] - s, 0, 255).astype(np.uint8)


def enhance(rgb):
    """scanner.py:55-76, every stage boundary uint8."""
    x = lab_to_rgb(clahe_lab(rgb_to_lab(rgb)))
    return sharpen(lab_to_rgb(nlm_lab(rgb_to_lab(x))))
