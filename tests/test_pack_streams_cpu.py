"""CPU: the byte layouts of the host weight packers (ocrvi_test_pack_stream), against the numpy restatements of tests/pack_refs.py and
against tests/golden/pack_streams.json, the SHA-256 of every case as the packers produced it BEFORE their shared steps (weight scale,
hi / lo split, quartet regrouping, row swizzle) were gathered into csrc/weight_pack.h; and the launchers' persistent_grid rule."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import pack_refs as R
from ocr_vi_invoice_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_streams.json")
FAMILIES = ("normal", "zero", "pow2", "below_pow2", "inf", "mixed", "index")
F16X2 = L.OCRVI_F16X2


def make_weights(shape, family, seed, k=-2):
    """one weight tensor of a family; pow2 / below_pow2: the largest magnitude is exactly 2^k / the fp32 just below it (and negative)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    w = (rng.standard_normal(n) * 0.05).astype(np.float32)
    if family == "zero":
        w[:] = 0
    elif family in ("pow2", "below_pow2"):
        top = np.float32(2.0 ** k)
        w = np.clip(w, -0.5 * top, 0.5 * top)
        w[n // 3] = -top if family == "pow2" else -np.nextafter(top, np.float32(0))
    elif family == "inf":
        w[n // 5] = np.inf
    elif family == "mixed":                                   # half of the weights 2^-20 of the others: their lo halves are subnormal fp16
        w *= np.where(rng.integers(0, 2, n) == 1, np.float32(2.0 ** -20), np.float32(1))
    elif family == "index":
        w = np.arange(n, dtype=np.float32)
    return w.reshape(shape)


# name -> (kind, d0, d1, shapes of (w0, w1 or None), restatement, rows per unit)
LAYOUTS = {
    "lin_x2_n32_k256": (0, 32, 256, ((32, 256), None), lambda a, b: R.lin_x2_stream(a), 256),
    "lin_x2_n64_k384": (0, 64, 384, ((64, 384), None), lambda a, b: R.lin_x2_stream(a), 384),
    "mlp_x2_d128": (1, 128, F16X2, ((512, 128), (128, 512)), R.mlp_x2_stream, 256),
    "mlp_x2_d256": (1, 256, F16X2, ((1024, 256), (256, 1024)), R.mlp_x2_stream, 512),
    "mlp_x2_d384": (1, 384, F16X2, ((1536, 384), (384, 1536)), R.mlp_x2_stream, 768),
    "mlp_f16_d128": (1, 128, L.OCRVI_F16, ((512, 128), (128, 512)), lambda a, b: R.mlp16_stream(a, b, "f16"), 128),
    "mlp_bf16_d128": (1, 128, L.OCRVI_BF16, ((512, 128), (128, 512)), lambda a, b: R.mlp16_stream(a, b, "bf16"), 128),
    "bneck_tail_w1": (2, 0, 0, ((256, 64), (64, 256)), R.bneck_tail_stream, 64),
    "bneck_tail_y_only": (2, 0, 0, ((256, 64), None), R.bneck_tail_stream, 64),
    "conv3_halo_64_64": (3, 64, 64, ((64, 64, 3, 3), None), lambda a, b: R.conv3_quartets(a, False), None),
    "dcn_pipe_64_64": (4, 64, 64, ((64, 64, 3, 3), None), lambda a, b: R.conv3_quartets(a, True), None),
}


def families_of(name):
    if name.startswith("mlp_") and "x2" not in name:
        return ("normal", "mixed")                           # plain 16-bit elements: no scale, no split
    return FAMILIES if name.startswith(("lin_x2", "mlp_x2", "bneck")) else FAMILIES[:-1]


CASES = [(n, f) for n in LAYOUTS for f in families_of(n)]


def weights_of(name, family):
    shapes = LAYOUTS[name][3]
    seed = CASES.index((name, family))
    w0 = make_weights(shapes[0], family, 2 * seed, k=-2)
    w1 = make_weights(shapes[1], family, 2 * seed + 1, k=3) if shapes[1] else None
    return w0, w1


def pack(name, w0, w1):
    """(bytes uint8, scales) of the library; the f16x2 lin / mlp streams carry their scales behind the units"""
    kind, d0, d1 = LAYOUTS[name][:3]
    lib = L.load()
    size, sc = C.c_size_t(0), (C.c_float * 2)()
    p1 = w1.ctypes.data if w1 is not None else None
    L.check(lib.ocrvi_test_pack_stream(kind, w0.ctypes.data, p1, d0, d1, None, 0, C.byref(size), sc))
    out = np.full(size.value + 64, 0xA5, np.uint8)
    L.check(lib.ocrvi_test_pack_stream(kind, w0.ctypes.data, p1, d0, d1, out.ctypes.data, size.value, C.byref(size), sc))
    assert (out[size.value:] == 0xA5).all(), "the hook wrote past the size it reported"
    got = out[:size.value]
    if kind == 0 or (kind == 1 and d1 == F16X2):
        nt = 4 if kind == 0 else 8
        return got, tuple(float(v) for v in got[-nt:].view(np.float32))
    return got, ((sc[0], sc[1]) if kind == 2 else (sc[0],) if kind >= 3 else ())


def record(name, family):
    w0, w1 = weights_of(name, family)
    got, scales = pack(name, w0, w1)
    kind, d0, d1 = LAYOUTS[name][:3]
    return {"kind": kind, "d0": d0, "d1": d1, "bytes": int(got.size), "sha256": hashlib.sha256(got.tobytes()).hexdigest(),
            "scales": [float(s).hex() for s in scales]}


def same_bytes(a, b):
    """byte equality, except that a NaN half (the lo half of an infinite weight: inf - inf) only has to be a NaN in both"""
    a, b = np.array(a), np.array(b)
    if a.size != b.size:
        return a, b
    ha, hb = a[:a.size // 2 * 2].view(np.float16), b[:b.size // 2 * 2].view(np.float16)
    nan = np.isnan(ha) & np.isnan(hb)
    ha[nan] = 0
    hb[nan] = 0
    return a, b


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_exactly_these_cases(golden):
    assert set(golden) == {f"{n}/{f}" for n, f in CASES}


@pytest.mark.parametrize("name,family", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_stream_equals_restatement_and_recorded_digest(name, family, golden):
    w0, w1 = weights_of(name, family)
    got, scales = pack(name, w0, w1)
    want, want_scales = LAYOUTS[name][4](w0, w1)
    f16x2 = not (name.startswith("mlp_") and "x2" not in name)
    print(name, family, "bytes", got.size, "scales", [float(s).hex() for s in scales])
    assert tuple(scales) == tuple(float(s) for s in want_scales)
    if family != "inf" or not f16x2:
        g, w = got, want
    else:
        g, w = same_bytes(got, want)
    assert g.size == w.size and np.array_equal(g, w), R.locate(g, w, rows_per_unit=LAYOUTS[name][5])
    if f16x2:                                                # what each family is there to show
        for s, t in zip(scales, (w0, w1)):
            if t is None:                                    # bneck_tail without the next conv1
                assert s == 1.0
                continue
            mx = float(np.abs(t).max())
            if family in ("zero", "inf"):
                assert s == 1.0
            else:
                assert 2.0 ** 13 <= mx / s < 2.0 ** 14 and np.frexp(s)[0] == 0.5
            if family == "pow2":
                assert mx / s == 2.0 ** 13
            if family == "below_pow2":
                assert mx / s == float(np.nextafter(np.float32(2.0 ** 14), np.float32(0)))
        if family == "zero":
            nt = 4 * len(scales) if LAYOUTS[name][0] < 2 else 0
            assert not got[:got.size - nt].any()
        if family == "mixed":
            units = got[:got.size // 32 * 32].view(np.float16)
            assert ((units != 0) & (np.abs(units) < 2.0 ** -14)).any(), "no subnormal lo half: the family does not test what it should"
    rec = golden[f"{name}/{family}"]
    assert rec["bytes"] == got.size and rec["scales"] == [float(s).hex() for s in scales]
    assert rec["sha256"] == hashlib.sha256(got.tobytes()).hexdigest()


@pytest.mark.parametrize("name,swz", [("lin_x2_n64_k384", R.swz128), ("mlp_x2_d128", R.swz128), ("bneck_tail_w1", R.swz_halo)])
def test_rows_are_stored_under_the_host_swizzle(name, swz):
    """rows 0 .. 63 of a unit: the library's host swizzle is the bit expression, and it is where the index-valued stream keeps position 0"""
    lib = L.load()
    s128, shalo = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    L.check(lib.ocrvi_test_swizzles(s128, shalo))
    assert list(s128) == [((r >> 1) & 1) | (((r >> 3) & 1) << 2) for r in range(64)]
    assert list(shalo) == [((r >> 1) & 1) | (((r >> 2) & 1) << 2) for r in range(64)]
    host = list(s128) if swz is R.swz128 else list(shalo)
    w0, w1 = weights_of(name, "index")
    got, scales = pack(name, w0, w1)
    # the unit part whose LDS rows 0 .. 63 are inspected, and the weight index of k-slot 0 .. 7 of each of those rows
    if name.startswith("lin_x2"):
        first, idx = 0, lambda r: 384 * (r % 32) + 32 * (r // 32) + np.arange(8)        # unit 0: row 32 ks + r = w[r][32 ks .. + 8]
    elif name.startswith("mlp_x2"):
        first = 2 * 256 - 128                                                            # unit 1's fc2 part: rows n = fc2[n][chunk 0]
        idx = lambda r: 512 * r + np.array([0, 1, 2, 3, 16, 17, 18, 19])
    else:
        first, idx = 0, lambda r: 64 * (r % 32) + 32 * (r // 32) + np.array([0, 1, 2, 3, 16, 17, 18, 19])   # B unit of group 0
    scale = 1.0 / scales[-1 if name.startswith("mlp_x2") else 0]
    rows = got[first * 128:(first + 64) * 128].reshape(64, 8, 16)
    for r in range(64):
        hi, lo = R.split(idx(r).astype(np.float32) * np.float32(scale))       # positions 0 and 1 of the row: stored at sw and sw ^ 1
        at = [s for s in range(8) if np.array_equal(rows[r, s], hi.view(np.uint8)) and np.array_equal(rows[r, s ^ 1], lo.view(np.uint8))]
        assert at == [host[r]], (name, r, at, host[r])


def test_persistent_grid_is_the_old_expression_and_balanced():
    lib = L.load()
    cdiv = lambda a, b: (a + b - 1) // b
    g = C.c_int32(0)
    for slots in (1, 2, 64, 128, 256, 512):
        for ntile in range(1, 601):
            L.check(lib.ocrvi_test_persistent_grid(ntile, slots, C.byref(g)))
            grid = g.value
            assert 1 <= grid <= min(ntile, slots)
            assert max(len(range(b, ntile, grid)) for b in (0, grid - 1)) <= cdiv(ntile, grid)
            assert cdiv(ntile, grid) * (grid - 1) < ntile              # the walk `tile += grid` leaves no workgroup idle ...
            assert cdiv(ntile, grid) == cdiv(ntile, min(ntile, slots))  # ... and none gets more than with every slot taken
            old = min(ntile, slots)                                     # the launchers' own lines before persistent_grid
            old = cdiv(ntile, cdiv(ntile, old))
            assert grid == old and grid == cdiv(ntile, cdiv(ntile, max(1, slots)))   # (gconv32's form: no min)


if __name__ == "__main__":                                   # regenerate the golden file from the library in use
    with open(GOLDEN, "w") as f:
        json.dump({f"{n}/{fam}": record(n, fam) for n, fam in CASES}, f, indent=1)
        f.write("\n")
