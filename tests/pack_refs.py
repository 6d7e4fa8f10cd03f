"""numpy restatements of the byte layouts the host weight packers hand to the f16x2 stream kernels (mlp_x2, lin_x2, bneck_tail), to
conv3_halo / dcn_pipe (the quartet form of pack_conv) and to the 16-bit fused MLP, written from the layout comments above each packer and
independently of the C++: gather, split, regroup and swizzle are index arithmetic on arrays, the scale is np.frexp.

Shared by all f16x2 layouts:
  scale    one power of two per layer that puts the largest |w| into [2^13, 2^14); 1 for an all-zero or non-finite tensor
  split    x = w * scale (fp32), hi = fp16(x), lo = fp16(x - hi)
  quartets the 8 consecutive k-slots 8 q .. 8 q + 7 of a row occupy 32 bytes: 16 bytes of their hi halves, then 16 bytes of their lo halves
  LDS rows a 128-byte row is eight 16-byte positions (2 q: hi, 2 q + 1: lo); position P is stored at P ^ swizzle(row)
"""
import numpy as np


def swz128(row):
    return ((row >> 1) & 1) | (((row >> 3) & 1) << 2)


def swz_halo(row):
    return ((row >> 1) & 1) | (((row >> 2) & 1) << 2)


def weight_scale(w):
    mx = np.abs(np.asarray(w, np.float32)).max()
    if not (mx > 0 and np.isfinite(mx)):
        return np.float32(1.0)
    _, e = np.frexp(mx)                                       # mx = m 2^e with m in [0.5, 1): mx 2^(14 - e) is in [2^13, 2^14)
    return np.float32(2.0 ** int(np.clip(14 - int(e), -100, 100)))


def split(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def quartets(x):
    """x [..., 8 G] fp32 (already scaled) -> uint8 [..., 32 G]: per 8 k-slots [8 hi | 8 lo]"""
    hi, lo = split(x)
    g = x.shape[:-1] + (x.shape[-1] // 8, 8)
    return np.ascontiguousarray(np.concatenate([hi.reshape(g), lo.reshape(g)], axis=-1)).view(np.uint8).reshape(x.shape[:-1] + (-1,))


def lds_rows(vals, sw):
    """vals [R][32] fp32 in the consumer's k-slot order (already scaled), sw [R] -> uint8 [R][128]"""
    R = vals.shape[0]
    pos = quartets(vals).reshape(R, 8, 16)
    out = np.empty_like(pos)
    out[np.arange(R)[:, None], np.arange(8)[None, :] ^ np.asarray(sw)[:, None]] = pos
    return out.reshape(R, 128)


def _tail(*scales):
    return (np.float32(1.0) / np.asarray(scales, np.float32)).view(np.uint8)


def lin_x2_stream(w):
    """w [N][K]: N / 32 units, each [K / 32][32 rows][128 B]; row r of unit u = output column 32 u + r, its K-step ks = w[.., 32 ks .. + 32];
    swz128 of the row index in the unit; then 1 / scale."""
    N, K = w.shape
    s = weight_scale(w)
    vals = (w.astype(np.float32) * s).reshape(N // 32, 32, K // 32, 32).transpose(0, 2, 1, 3).reshape(-1, 32)
    row = np.arange(vals.shape[0]) % (K // 32 * 32)
    return np.concatenate([lds_rows(vals, swz128(row)).ravel(), _tail(s)]), (1.0 / s,)


def mlp_x2_stream(w1, w2):
    """fc1 [4D][D], fc2 [D][4D].  Unit k = 0 .. 4 D / 32: [D / 32][32 hidden rows][128 B] of fc1's chunk k (zeros for the last unit), then [D output
    rows][128 B] of fc2's chunk k - 1 (zeros for the first) with position 8 g + j <-> hidden 16 (j >> 2) + 4 g + (j & 3); swz128 of the row
    index in its part; then 1 / s1, 1 / s2."""
    H4, D = w1.shape
    NCH, KS = H4 // 32, D // 32
    s1, s2 = weight_scale(w1), weight_scale(w2)
    a = (w1.astype(np.float32) * s1).reshape(NCH, 32, KS, 32).transpose(0, 2, 1, 3).reshape(NCH, KS * 32, 32)
    pos = np.arange(32)
    hid = 16 * ((pos & 7) >> 2) + 4 * (pos >> 3) + (pos & 3)
    b = (w2.astype(np.float32) * s2).reshape(D, NCH, 32)[:, :, hid].transpose(1, 0, 2)
    a = np.concatenate([a, np.zeros_like(a[:1])])
    b = np.concatenate([np.zeros_like(b[:1]), b])
    vals = np.concatenate([a, b], axis=1)                     # [NCH + 1][KS * 32 + D][32]
    sw = np.tile(np.concatenate([swz128(np.arange(KS * 32)), swz128(np.arange(D))]), NCH + 1)
    return np.concatenate([lds_rows(vals.reshape(-1, 32), sw).ravel(), _tail(s1, s2)]), (1.0 / s1, 1.0 / s2)


def _to16(x, dtype):
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).view(np.uint8)
    u = x.view(np.uint32)                                      # bf16, round to nearest even (finite values)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.uint8)


def mlp16_stream(w1, w2, dtype):
    """The 16-bit fused MLP's pieces (plain elements, no scale).  Hidden chunks of 64: G1(hc) = D / 128 pieces of [2 K-steps][64 hidden rows][64 of
    K]; G2(hc) = D / 128 pieces of [128 output rows][64] with position 16 g + 8 h + j <-> hidden 16 (2 h + (j >> 2)) + 4 g + (j & 3).  Order:
    G1(0), G1(1), then G1(c + 1), G2(c - 1) for c = 1 .. NCH - 2, then G2(NCH - 2), G2(NCH - 1)."""
    H4, D = w1.shape
    NCH, NP = H4 // 64, D // 128
    pos = np.arange(64)
    hid = 16 * (2 * ((pos >> 3) & 1) + ((pos & 7) >> 2)) + 4 * (pos >> 4) + (pos & 3)

    def g1(hc):
        return w1[64 * hc:64 * hc + 64].reshape(64, NP, 2, 64).transpose(1, 2, 0, 3).ravel()

    def g2(hc):
        return w2[:, 64 * hc:64 * hc + 64][:, hid].ravel()   # [p2][n] = output row 128 p2 + n

    parts = [g1(0), g1(1)]
    for c in range(1, NCH - 1):
        parts += [g1(c + 1), g2(c - 1)]
    parts += [g2(NCH - 2), g2(NCH - 1)]
    return _to16(np.concatenate(parts), dtype), ()


_KSLOT = np.array([(4 * g + e) if e < 4 else (16 + 4 * g + e - 4) for g in range(4) for e in range(8)])


def bneck_tail_stream(w3, w1):
    """w3 [256][64], w1 [64][256] or None.  Per group q of 32 conv3 channels: a B unit of 64 rows R = 32 j + n = channel 32 q + n over input
    channels 32 j + .., then (with w1) a C unit of 64 rows m over input channels 32 q + ..; lane group g's eight k-slots are channels
    base + 4 g + e and base + 16 + 4 g + e (e = 0 .. 3); swz_halo of the row."""
    s3 = weight_scale(w3)
    s1 = weight_scale(w1) if w1 is not None else np.float32(1.0)
    x3 = w3.astype(np.float32) * s3
    sw = swz_halo(np.arange(64))
    units = []
    for q in range(8):
        rows = np.stack([x3[32 * q + n, 32 * j + _KSLOT] for j in range(2) for n in range(32)])
        units.append(lds_rows(rows, sw))
        if w1 is not None:
            units.append(lds_rows((w1.astype(np.float32) * s1)[:, 32 * q + _KSLOT], sw))
    return np.concatenate(units).ravel(), (1.0 / s3, 1.0 / s1)


def conv3_quartets(w, dcn):
    """w [Co][C][3][3], Co a multiple of the column tile (64 for 33 .. 64 channels).  Row n = output channel, K order (tap, channel) for
    conv3_halo and (block of 32 channels, tap, channel) for dcn_pipe; plain quartets over consecutive k, no swizzle."""
    Co, C = w.shape[:2]
    s = weight_scale(w)
    x = (w.astype(np.float32) * s).reshape(Co, C, 9).transpose(0, 2, 1)                # [n][tap][c]
    if dcn:
        x = x.reshape(Co, 9, C // 32, 32).transpose(0, 2, 1, 3)
    return quartets(x.reshape(Co, 9 * C)).ravel(), (1.0 / s,)


def locate(got, want, row_bytes=128, rows_per_unit=None):
    """the first differing byte as text: (unit, row, 16-byte position, byte) where the stream is made of 128-byte rows"""
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size:
        return f"sizes differ: {got.size} != {want.size}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    row = i // row_bytes
    unit = f"unit {row // rows_per_unit}, row {row % rows_per_unit}" if rows_per_unit else f"row {row}"
    return f"{bad.size} bytes differ, first at byte {i}: {unit}, position {i % row_bytes // 16}, byte {i % 16}: {got[i]} != {want[i]}"
