"""Skew estimate, host half (include/ocrvi.h, "Skew estimate"): ocrvi_skew_pick, ocrvi_skew_quad and ocrvi_skew_sizes against the Python
statement in tests/skew_ref.py; the statement itself against the definition pixel by pixel, on rotated synthetic invoices, and against its
own mutants.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import skew_ref as SR
import warp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("ocrvi_skew_sizes", "ocrvi_skew_scores_pages", "ocrvi_skew_edges_u8", "ocrvi_skew_scores", "ocrvi_skew_pick", "ocrvi_skew_quad")
K = SR.K


def _lib():
    from ocr_vi_invoice_amd import _lib
    return _lib


def test_exports_header_and_binding_agree():
    import ocr_vi_invoice_amd as pkg
    L = _lib()
    lib = L.load()
    with open(os.path.join(HERE, "..", "include", "ocrvi.h")) as f:
        header = f.read()
    for n in NEW_EXPORTS:
        assert n in L.EXPORTS and hasattr(lib, n) and re.search(r"\bint " + n + r"\(", header), n
    for name, v in (("K", SR.K), ("SHIFT", SR.SHIFT), ("FLOOR", SR.FLOOR), ("ANGLES", SR.ANGLES)):
        assert f"#define OCRVI_SKEW_{name} {v}\n" in header
    assert (L.SKEW_K, L.SKEW_ANGLES) == (SR.K, SR.ANGLES)
    assert lib.ocrvi_abi_version() == 5 == L.ABI_VERSION
    for n in ("Skew", "estimate_skew", "estimate_skews", "skew_quad", "deskew"):
        assert callable(getattr(pkg, n))


# ---------------------------------------------------------------------------------------------------- pick
def _scores(fill, **at):
    s = np.full(SR.ANGLES, fill, np.uint64)
    for k, v in at.items():
        s[int(k.replace("m", "-").replace("p", "")) + K] = v
    return s


PICKS = {
    # name: (scores, the k to expect)
    "a_single_maximum": (_scores(10, m37=99), -37),
    "a_tie_at_plus_and_minus_k": (_scores(10, m5=99, p5=99), 5),
    "a_tie_at_different_k": (_scores(10, m3=99, p40=99, m90=99), -3),
    "a_tie_with_zero": (_scores(10, p0=99, p1=99, m1=99), 0),
    "all_equal": (_scores(7), 0),
    "all_zero": (_scores(0), 0),
    "s0_zero_best_positive": (_scores(0, m128=5), -128),
    "above_2_53": (_scores(2 ** 53 + 1, p0=2 ** 53 + 3, p128=2 ** 53 + 4, m127=2 ** 53 + 2), 128),
    "above_2_53_neighbours_a_double_cannot_tell_apart": (_scores(1, p0=3, m2=2 ** 53 + 1, p9=2 ** 53 + 2), 9),
}


@pytest.mark.parametrize("name", list(PICKS))
def test_pick_equals_the_restatement(name):
    from ocr_vi_invoice_amd import pipeline
    scores, want_k = PICKS[name]
    ref, got = SR.pick(scores), pipeline.skew_pick(scores)
    assert isinstance(got, pipeline.Skew) and got.k == ref.k == want_k
    assert got.angle == pytest.approx(ref.angle, rel=1e-12, abs=0)
    assert got.gain == ref.gain if math.isinf(ref.gain) else got.gain == pytest.approx(ref.gain, rel=1e-12, abs=0)
    assert abs(got.angle - math.degrees(math.atan2(got.k, 512))) < 1e-12
    if name == "all_zero":
        assert got.gain == 1.0
    if name == "s0_zero_best_positive":
        assert got.gain == math.inf
    if name == "above_2_53":
        assert got.gain == float(2 ** 53 + 4) / float(2 ** 53 + 3)


# ---------------------------------------------------------------------------------------------------- quad
SHAPES = ((960, 1280), (1280, 960), (100, 4000), (8, 8))
SLOPES = (-128, -1, 0, 1, 37, 128)


@pytest.mark.parametrize("h,w", SHAPES)
def test_quad_equals_the_restatement_bit_for_bit(h, w):
    from ocr_vi_invoice_amd import pipeline
    for k in SLOPES:
        got, ref = pipeline.skew_quad(h, w, k), SR.quad(h, w, k)
        assert got.dtype == np.float64 and got.shape == (4, 2) and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (k, got, ref)
        # the upright rectangle that encloses the page: right angles, every page corner inside, two of them on each pair of opposite sides
        u, v = got[1] - got[0], got[3] - got[0]
        assert abs(u @ v) <= 1e-9 * (u @ u) and np.allclose(got[0] + u + v, got[2], atol=1e-9)
        assert math.atan2(u[1], u[0]) == pytest.approx(math.atan(k / 512.0), abs=1e-12)
        corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64) - got[0]
        a, b = corners @ u / (u @ u), corners @ v / (v @ v)
        assert a.min() == pytest.approx(0, abs=1e-9) and a.max() == pytest.approx(1, abs=1e-9)
        assert b.min() == pytest.approx(0, abs=1e-9) and b.max() == pytest.approx(1, abs=1e-9)
        # four_point_transform takes it, in the order given
        m_fwd, m_inv, ow, oh = pipeline.four_point_geometry(got)
        rect, _, rw, rh, _, _ = warp_ref.four_point_geometry(got)
        assert np.array_equal(rect, got.astype(np.float32)) and (ow, oh) == (rw, rh)
        assert abs(ow - math.hypot(*u)) <= 1 and abs(oh - math.hypot(*v)) <= 1
        if k == 0:
            assert np.array_equal(got, [[0, 0], [w, 0], [w, h], [0, h]]) and (ow, oh) == (w, h)
    with pytest.raises(ValueError):
        pipeline.skew_quad(h, w, 129)
    with pytest.raises(ValueError):
        pipeline.skew_quad(0, w, 1)


def test_sizes_refuses_what_lies_outside_the_bounds():
    lib, n = _lib().load(), ctypes.c_size_t(0)
    assert lib.ocrvi_skew_sizes(3, 500, 666, ctypes.byref(n)) == 0 and n.value >= 3 * 2 * 500 * 666
    one = ctypes.c_size_t(0)
    assert lib.ocrvi_skew_sizes(1, 37, 101, ctypes.byref(one)) == 0 and one.value >= 37 * 101 + 40 * 101
    for bad in ((0, 500, 666), (65536, 500, 666), (1, 7, 666), (1, 513, 666), (1, 500, 7), (1, 500, 8193)):
        assert lib.ocrvi_skew_sizes(*bad, ctypes.byref(n)) == -1, bad
    assert lib.ocrvi_skew_sizes(1, 500, 666, None) == -1


# ---------------------------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_equals_the_definition_pixel_by_pixel():
    rng = np.random.default_rng(3200)
    for h, ww in ((8, 8), (11, 23), (30, 14)):
        E = rng.integers(0, 256, (h, ww), dtype=np.uint8)
        E[rng.random((h, ww)) < 0.4] = 0
        sc = SR.scores(E)
        for k in (-128, -77, -2, -1, 0, 1, 2, 50, 127, 128):
            P = SR.profile_brute(E, k)
            r_min, Pk = SR.profile(E, k)
            assert {r: v for r, v in P.items() if v} == {r_min + i: int(v) for i, v in enumerate(Pk) if v}
            assert int(sc[k + K]) == sum(v * v for v in P.values())
    assert np.array_equal(SR.scores_constant(40, 300, 255), SR.scores(np.full((40, 300), 255, np.uint8)))
    assert int(SR.scores_constant(512, 8192, 255)[K]) == 512 * (255 * 8192) ** 2
    g = SR.grey_cases()[1]
    e = SR.edges(g)
    for i, j in ((0, 0), (3, 0), (5, 100), (36, 100), (7, 50), (8, 1), (8, 99)):
        d = abs(int(g[i, min(j + 1, 100)]) - int(g[i, max(j - 1, 0)]))
        assert int(e[i, j]) == (d if d >= 8 else 0)
    assert {7, 8, 9} <= set(np.abs(g[0::2, 3:-2].astype(int) - g[0::2, 1:-4].astype(int)).reshape(-1).tolist())
    assert (e[0::2, 2:-2] <= 9).all() and 7 not in e and 8 in e and 9 in e


_PAGES = {}


def _page(which):
    if which not in _PAGES:
        from ocr_vi_invoice_amd import synth
        _PAGES[which] = synth.make_invoice(*((1, 960, 1280, 30), (2, 1280, 960, 40))[which])[0]
    return _PAGES[which]


@pytest.mark.parametrize("enclose", [True, False], ids=["enclosing_canvas", "same_size_crop"])
@pytest.mark.parametrize("degrees", [0, 0.5, -1.3, 3, -7, 12, -13])
@pytest.mark.parametrize("which", [0, 1], ids=["960x1280", "1280x960"])
def test_the_estimator_recovers_a_known_angle(which, degrees, enclose):
    page = _page(which)
    img = page if degrees == 0 else SR.rotated(page, degrees, enclose)
    skew = SR.estimate(img, 500)
    print(f"page {which} at {degrees} degrees, enclose={enclose}: k = {skew.k} ({512 * math.tan(math.radians(degrees)):.2f}), gain = {skew.gain:.3f}")
    if degrees == 0:
        assert skew.k == 0 and skew.gain == 1.0
    else:
        assert abs(skew.k - 512 * math.tan(math.radians(degrees))) <= 2
        assert skew.gain > 1.0 and skew.angle == pytest.approx(degrees, abs=2 * 0.112)


# ---------------------------------------------------------------------------------------------------- mutants
def _shows(mutant):
    """The first input of the GPU tests on which the mutant changes a score."""
    if mutant in ("floor_dropped", "border_wrapped"):
        for g in SR.grey_cases():
            if not np.array_equal(SR.scores(SR.edges(g, mutant)), SR.scores(SR.edges(g))):
                return g.shape
        return None
    for name, E in SR.score_cases().items():
        if name != "all_255_512x8192" and not np.array_equal(SR.scores(E, mutant), SR.scores(E)):
            return name
    return None


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_every_mutant_changes_a_score_on_the_gpu_tests_inputs(mutant):
    assert _shows(mutant) is not None
