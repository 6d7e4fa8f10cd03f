"""The character n-gram model's host entries (``ocrvi_lm_build`` / ``ocrvi_lm_score`` / the validator behind ``ocrvi_lm_create``) against the
restatement of tests/ctclm_ref.py, bit for bit; the trainer and its normalisation; the reference beam search against brute force, its
mutants and the separation condition on the shared case list (tests/ctclm_cases.py); the C ABI's text and the Python layer's host-side
errors.  No GPU."""
import ctypes as C
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctclm_cases as LC  # noqa: E402
import ctclm_ref as LR  # noqa: E402

from ocr_vi_invoice_amd import _lib  # noqa: E402
from ocr_vi_invoice_amd import lm as LM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ocrvi_lm_build", "ocrvi_lm_score", "ocrvi_lm_create", "ocrvi_lm_destroy", "ocrvi_ctc_beam_lm_workspace_bytes", "ocrvi_ctc_beam_lm")
NAMES = [c[0] for c in LC.CASES]
EINVAL = -1

# mutant -> cases whose expected device output it changes (each by an id, or by more than 1e-6 in a score: the GPU test holds 1e-9)
MUTANT_CASES = {
    "no_backoff": ("brute_T5_o2_a2.0_b0.0", "one_hot_lm", "golden_W8"),
    "ctx_not_truncated": ("brute_T5_o1_a0.5_b0.0", "brute_T6_o3_a0.5_b0.7", "T64_C40_W16"),
    "no_bos": ("decide_a1", "brute_T5_o2_a0.5_b-0.7", "text_like_W8"),
    "lm_on_stay": ("one_hot_lm", "decide_a1", "golden_W8"),
    "len_on_stay": ("tie_R_equal", "one_hot_lm", "text_like_W8"),
    "repeat_wrong_ctx": ("brute_T5_o2_a2.0_b0.0", "C2_T20_W8", "text_like_W8"),
    "unk_ninf": ("unk_T10_C5_W8", "collide_T12_C40_W8"),
    "rank_by_s": ("decide_a1", "tie_R_equal", "golden_W8"),
    # the two associations differ by one rounding, 1e-16 relative: only an exact tie that one of them breaks tells them apart
    "assoc": ("tie_assoc",),
}


def _arrays(grams):
    ids = np.full((len(grams), 6), -1, np.int32)
    lens = np.zeros(len(grams), np.int32)
    for i, (g, _, _) in enumerate(grams):
        lens[i] = len(g)
        ids[i, :min(len(g), 6)] = g[:6]
    return ids, lens, np.array([g[1] for g in grams], np.float32), np.array([g[2] for g in grams], np.float32)


def lib_build(grams, order, num_classes, bos, unk):
    """(rc, blob bytes or None) of ocrvi_lm_build: the size query, then the build."""
    lib = _lib.load()
    ids, lens, lp, bo = _arrays(grams)
    args = (ids.ctypes.data, lens.ctypes.data, lp.ctypes.data, bo.ctypes.data, len(grams), order, num_classes, bos, unk)
    n = C.c_size_t(0)
    rc = lib.ocrvi_lm_build(*args, None, 0, C.byref(n))
    if rc:
        return rc, None
    buf = C.create_string_buffer(n.value)
    assert lib.ocrvi_lm_build(*args, buf, n.value - 1, C.byref(n)) == -3          # OCRVI_ENOMEM
    assert lib.ocrvi_lm_build(*args, buf, n.value, C.byref(n)) == 0
    return 0, buf.raw


def lib_score(blob, ids):
    lib = _lib.load()
    a = np.asarray(ids, np.int32)
    total = C.c_double(7.0)
    terms = np.full(max(len(a), 1), 7.0)
    rc = lib.ocrvi_lm_score(blob, len(blob), a.ctypes.data, len(a), C.byref(total), terms.ctypes.data)
    return rc, total.value, terms[:len(a)].tolist()


def _bits(x):
    return struct.pack("<d", x)


def _strings(t: LR.Table, seed, n=40, maxlen=9):
    rng = np.random.default_rng(seed)
    labels = [c for c in range(t.C) if c != t.bos]
    out = [(), (labels[0],), (labels[-1],) * 3]
    for g, _, _ in t.list[:: max(1, len(t.list) // 60)]:                # strings that walk the table's own grams
        out.append(tuple(c for c in g if c != t.bos))
    for _ in range(n):
        out.append(tuple(int(c) for c in rng.choice(labels, int(rng.integers(1, maxlen)))))
    return out


# ---------------------------------------------------------------------------------------------------- build and score
TABLES = ("hand3_o1", "hand3_o2", "hand3_o3", "hand3_o2_blank2", "unk5_o2", "collide40", "trained_o2", "trained_o4", "order6_C1024", "tie8",
          "rand40_o3_blank39")


@pytest.mark.parametrize("name", TABLES)
def test_build_and_score_equal_the_reference_bit_for_bit(name):
    t = LC.table(name)
    rc, blob = lib_build(t.list, t.order, t.C, t.bos, t.unk)
    assert rc == 0 and blob == t.blob()                                 # header, capacity, home slots and probe order
    for l in _strings(t, 5):
        want_terms = []
        want = t.g(l, want_terms)
        rc, got, terms = lib_score(blob, l)
        assert rc == 0 and _bits(got) == _bits(want) and [_bits(x) for x in terms] == [_bits(x) for x in want_terms], (name, l, got, want)


def test_probe_is_the_dict_and_row_is_cond():
    """The reference's own two forms agree: probing the blob's slots finds exactly the grams given, and the vectorised ``row`` the beam
    search uses holds ``cond``'s values."""
    rng = np.random.default_rng(3)
    for name in ("hand3_o3", "collide40", "order6_C1024", "trained_o4", "unk5_o2"):
        t = LC.table(name)
        assert all(t.probe(LR.key(g)) == (lp, bo) for g, lp, bo in t.list)
        labels = [c for c in range(t.C) if c != t.bos]
        for _ in range(200):
            g = tuple(int(c) for c in rng.choice(labels, int(rng.integers(1, t.order + 1))))
            assert t.probe(LR.key(g)) == t.grams.get(g)
        for l in _strings(t, 9, n=10):
            h = t.ctx(l)
            row = t.row(h)
            assert all(_bits(float(row[c])) == _bits(t.cond(h, c)) for c in labels[:: max(1, len(labels) // 50)]), (name, l)


def test_contexts_shorter_than_the_order_and_the_backoff_chain_by_hand():
    # order 4; (1, 2, 3) backs off through every level to the unigram of 4; 5 has no unigram
    grams = [((1,), -1.0, -0.25), ((2,), -1.5, -0.5), ((3,), -2.0, -0.125), ((4,), -3.0, 0.0), ((0,), 0.0, -0.75), ((0, 1), -0.5, -2.0),
             ((1, 2), -0.625, -4.0), ((2, 3), -0.875, -8.0), ((0, 1, 2), -0.0625, -16.0), ((1, 2, 3), -0.03125, -32.0), ((0, 1, 2, 3), -0.015625, 0.0)]
    t = LR.Table(grams, 4, 6, 0, -10.0)
    rc, blob = lib_build(grams, 4, 6, 0, -10.0)
    assert rc == 0 and blob == t.blob()
    # (1): BOS 1 -> -0.5; (1,2): BOS 1 2 -> -0.0625; (1,2,3): the 4-gram -> -0.015625; then 4 after (1,2,3): -32 -8 -0.125 + -3
    assert lib_score(blob, (1, 2, 3, 4)) == (0, -0.5 - 0.0625 - 0.015625 + (-32.0 - 8.0 - 0.125 - 3.0), [-0.5, -0.0625, -0.015625, -43.125])
    assert t.g((1, 2, 3, 4)) == -43.703125
    # a missing unigram: every level's weight, then unk_lp; at the line start only BOS backs off
    assert lib_score(blob, (1, 2, 3, 5))[2][3] == -32.0 - 8.0 - 0.125 - 10.0 and lib_score(blob, (5,)) == (0, -10.75, [-10.75])
    assert lib_score(blob, ()) == (0, 0.0, [])
    # a context whose longer forms are absent is skipped without a weight: (4, 1) -> (1, 2) matches at level 1 after no weight for (4, 1)
    assert lib_score(blob, (4, 1, 2))[2] == [-3.75, -1.0, -0.625]


def test_ids_at_the_ends_of_the_key_fields_at_order_6():
    """0 (BOS, first only), 1 and 1023 in every position of a 6-gram: the 10-bit fields and the length tag do not run into each other."""
    grams, want = [], {}
    for pos in range(6):
        for v in (0, 1, 1023) if pos == 0 else (1, 1023):
            g = [500 + pos] * 6
            g[pos] = v
            grams.append((tuple(g), -1.0 - pos - v / 1024.0, 0.0))
    grams += [((1023,) * k, -0.5 * k, -0.25) for k in range(1, 7)] + [((1,) * k, -0.75 * k, -0.125) for k in range(1, 6)]
    t = LR.Table(grams, 6, 1024, 0, -9.0)
    rc, blob = lib_build(grams, 6, 1024, 0, -9.0)
    assert rc == 0 and blob == t.blob()
    assert all(LR.key(g) >> 60 == len(g) and LR.key(g) < (1 << 63) for g, _, _ in grams) and len({LR.key(g) for g, _, _ in grams}) == len(grams)
    for g, lp, _ in grams:
        l = tuple(c for c in g if c != 0)
        rc, total, terms = lib_score(blob, l)
        assert rc == 0 and _bits(total) == _bits(t.g(l))
        if len(g) == 6 and g[0] != 0:
            assert _bits(lib_score(blob, (7,) + l)[2][-1]) == _bits(float(np.float32(lp)))     # the 6-gram itself, after any character
    assert lib_score(blob, (1023,) * 8)[2][-1] == -3.0                    # the 6-gram of 1023s


def test_a_table_at_exactly_half_load_and_a_wrapping_probe_chain():
    t = LC.table("collide40")
    assert len(t.list) == 8 and t.log2cap == 4 and all(LR.home(LR.key(g), 4) == 14 for g, _, _ in t.list)
    assert [i for i, k in enumerate(t.keys) if k] == [0, 1, 2, 3, 4, 5, 14, 15]          # round the end
    grams = [((c,), -0.125 * c, 0.0) for c in range(1, 17)]             # 16 entries -> 32 slots
    rc, blob = lib_build(grams, 1, 20, 0, -4.0)
    assert rc == 0 and len(blob) == 48 + 16 * 32 and blob == LR.Table(grams, 1, 20, 0, -4.0).blob()
    rc, blob = lib_build([], 1, 2, 0, -4.0)                               # no gram at all: two empty slots, everything is unk_lp
    assert rc == 0 and len(blob) == 48 + 32 and lib_score(blob, (1, 1)) == (0, -8.0, [-4.0, -4.0])


# ---------------------------------------------------------------------------------------------------- rejected inputs
GOOD = [((1,), -1.0, -0.5), ((2,), -1.5, 0.0), ((0,), 0.0, -0.25), ((0, 1), -0.5, 0.0), ((1, 2), -0.75, 0.0)]


@pytest.mark.parametrize("what,grams,order,num_classes,bos,unk", [
    ("a gram twice", GOOD + [((1, 2), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("id >= num_classes", GOOD + [((4,), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("negative id", GOOD + [((-1, 1), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("BOS second", GOOD + [((1, 0), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("BOS last of three", GOOD + [((1, 2, 0), -0.1, 0.0)], 3, 4, 0, -5.0),
    ("blank predicted", [((0,), -0.5, 0.0)], 2, 4, 0, -5.0),
    ("blank predicted, blank 3", [((3,), -0.5, 0.0)], 2, 4, 3, -5.0),
    ("lp inf", GOOD + [((2, 2), -math.inf, 0.0)], 2, 4, 0, -5.0),
    ("lp nan", GOOD + [((2, 2), math.nan, 0.0)], 2, 4, 0, -5.0),
    ("bo inf", GOOD + [((2, 2), -0.5, math.inf)], 2, 4, 0, -5.0),
    ("unk nan", GOOD, 2, 4, 0, math.nan),
    ("unk inf", GOOD, 2, 4, 0, -math.inf),
    ("order 0", GOOD[:2], 0, 4, 0, -5.0),
    ("order 7", GOOD, 7, 4, 0, -5.0),
    ("gram longer than the order", GOOD + [((1, 2, 1), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("empty gram", GOOD + [((), -0.1, 0.0)], 2, 4, 0, -5.0),
    ("num_classes 1", [], 1, 1, 0, -5.0),
    ("num_classes 1025", GOOD, 2, 1025, 0, -5.0),
    ("bos outside", GOOD, 2, 4, 4, -5.0),
])
def test_build_rejects(what, grams, order, num_classes, bos, unk):
    rc, blob = lib_build(grams, order, num_classes, bos, unk)
    assert rc == EINVAL and blob is None and _lib.last_error().startswith("lm_build:"), (what, _lib.last_error())


def test_build_accepts_what_is_legal():
    assert lib_build(GOOD, 2, 4, 0, -5.0)[0] == 0
    assert lib_build(GOOD + [((0, 2), 0.5, 3.0)], 2, 4, 0, 1.0)[0] == 0      # positive logs are finite floats
    assert _lib.load().ocrvi_lm_build(None, None, None, None, 0, 1, 4, 0, -5.0, None, 0, None) == EINVAL


def _corrupt(blob, off, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def test_validator_rejects_every_corrupt_blob():
    lib = _lib.load()
    t = LR.Table(GOOD, 2, 4, 0, -5.0)
    blob = t.blob()
    assert len(blob) == 48 + 16 * 16 and lib_score(blob, (1, 2))[0] == 0
    used = [i for i, k in enumerate(t.keys) if k]
    free = [i for i, k in enumerate(t.keys) if not k]
    s0, e0 = 48 + 16 * used[0], 48 + 16 * free[0]
    k0 = t.keys[used[0]]
    bad = {
        "truncated": blob[:-1], "one slot short": blob[:-16], "header only": blob[:48], "shorter than the header": blob[:40], "empty": b"",
        "one byte long": blob + b"\0",
        "magic": _corrupt(blob, 0, "<I", 0x12345678), "version": _corrupt(blob, 4, "<I", 2),
        "order 0": _corrupt(blob, 8, "<i", 0), "order 7": _corrupt(blob, 8, "<i", 7), "order below a key's length": _corrupt(blob, 8, "<i", 1),
        "num_classes 1": _corrupt(blob, 12, "<i", 1), "num_classes below an id": _corrupt(blob, 12, "<i", 2),
        "num_classes 1025": _corrupt(blob, 12, "<i", 1025),
        "bos outside": _corrupt(blob, 16, "<i", 4), "bos that makes a label BOS": _corrupt(blob, 16, "<i", 2),
        "log2cap 0": _corrupt(blob, 20, "<i", 0), "log2cap against the size": _corrupt(blob, 20, "<i", 5), "log2cap 41": _corrupt(blob, 20, "<i", 41),
        "entry count": _corrupt(blob, 24, "<Q", 4), "entry count past half": _corrupt(blob, 24, "<Q", 9),
        "unk nan": _corrupt(blob, 32, "<d", math.nan), "unk inf": _corrupt(blob, 32, "<d", math.inf),
        "length tag 0": _corrupt(blob, s0, "<Q", k0 & ((1 << 60) - 1)), "length tag 7": _corrupt(blob, s0, "<Q", (k0 & ((1 << 60) - 1)) | (7 << 60)),
        "bit 63": _corrupt(blob, s0, "<Q", k0 | (1 << 63)), "bits beyond the symbols": _corrupt(blob, s0, "<Q", k0 | (1 << 45)),
        "lp nan": _corrupt(blob, s0 + 8, "<f", math.nan), "bo inf": _corrupt(blob, s0 + 12, "<f", math.inf),
        "a key where no probe finds it": _corrupt(_corrupt(blob, s0, "<Q", 0), e0, "<Q", k0) if LR.home(k0, 4) != free[0] else blob[:47],
        "a key twice": _corrupt(blob, 24, "<Q", 6)[:e0] + struct.pack("<Qff", k0, 0.0, 0.0) + blob[e0 + 16:],
    }
    full = LR.Table([((c,), -1.0, 0.0) for c in range(1, 9)], 1, 10, 0, -5.0)       # 8 entries in 16 slots; made full by hand below
    fb = bytearray(full.blob())
    for i, k in enumerate(full.keys):
        if not k:
            struct.pack_into("<Qff", fb, 48 + 16 * i, (1 << 60) | 9, -1.0, 0.0)        # the same legal key in every empty slot
    struct.pack_into("<Q", fb, 24, 16)
    bad["no empty slot"] = bytes(fb)
    h = C.c_void_p()
    for what, b in bad.items():
        rc, total, _ = lib_score(b, (1, 2))
        assert rc == EINVAL and total == 7.0 and _lib.last_error().startswith("lm_score:"), (what, rc, _lib.last_error())
        assert lib.ocrvi_lm_create(0, b, len(b), C.byref(h)) == EINVAL and not h.value and _lib.last_error().startswith("lm_create:"), what
    assert lib.ocrvi_lm_create(0, blob, len(blob), None) == EINVAL and lib.ocrvi_lm_create(0, None, 0, C.byref(h)) == EINVAL
    # ids that are no labels
    for ids in ((0,), (1, 0), (4,), (-1,)):
        assert lib_score(blob, ids)[0] == EINVAL, ids
    lib.ocrvi_lm_destroy(None)                                           # a no-op


# ---------------------------------------------------------------------------------------------------- the trainer
LINES = [LC.TOK.encode_one(t) for t in LR.synthetic_lines(7, 300)]


@pytest.mark.parametrize("order", [1, 2, 4])
def test_trainer_equals_its_restatement(order):
    got, unk = LM.train_ngrams(LINES, order, LC.TOK.num_classes, 0, 0.75)
    want, wunk = LR.train(LINES, order, LC.TOK.num_classes, 0, 0.75)
    assert unk == wunk and got == want and all(len(g) <= order for g in got)
    assert all((c,) in got for c in range(1, LC.TOK.num_classes))      # every class has a unigram
    m = LM.CharLM.train(LR.synthetic_lines(7, 300), LC.TOK, order)
    t = LR.Table([(g, lp, bo) for g, (lp, bo) in want.items()], order, LC.TOK.num_classes, 0, wunk)
    assert m.blob == t.blob() and len(m) == len(want)
    assert _bits(m.score("hoá đơn 10%")) == _bits(t.g(LC.TOK.encode_one("hoá đơn 10%")))


@pytest.mark.parametrize("order", [2, 4])
def test_trainer_normalises(order):
    """sum over c != blank of exp(lm(c | h)) = 1 for seen contexts, unseen ones and the line start.  On the trainer's float64 values the
    bound is 1e-12: float64 summation of at most 231 terms of magnitude <= 1 (2.6e-14) beside the rounding of one log / exp pair and of
    the 1 - sum in bo per level (a few 1e-16 each, times the 1 / (1 - sum) <= ~1e3 it is divided by).  The table stores float32: each of the
    at most ``order`` terms of a score moves by <= 2^-24 of its size (<= 16), so the stored model is held to 1e-5."""
    grams, unk = LM.train_ngrams(LINES, order, LC.TOK.num_classes, 0, 0.75)
    t = LR.Table([(g, lp, bo) for g, (lp, bo) in grams.items()], order, LC.TOK.num_classes, 0, unk)
    labels = range(1, LC.TOK.num_classes)
    rng = np.random.default_rng(order)
    seen = [g for g in grams if len(g) == order - 1 and g[0] != 0]
    contexts = [(0,)] + [seen[int(i)] for i in rng.integers(0, len(seen), 12)]
    contexts += [g for g in grams if len(g) == min(order - 1, 2) and g[0] == 0][:4]             # BOS + one character
    contexts += [tuple(int(c) for c in rng.integers(2, LC.TOK.num_classes, order - 1)) for _ in range(6)]     # unseen
    contexts += [(1,) * (order - 1), seen[0][:-1] + (1,)]                                       # the pad id: never seen
    worst64 = worst32 = 0.0
    for h in contexts:
        h = h[len(h) - min(len(h), order - 1):]
        p64 = math.fsum(math.exp(LM.cond_log_prob(grams, h, c, unk)) for c in labels)
        p32 = math.fsum(math.exp(t.cond(h, c)) for c in labels)
        worst64, worst32 = max(worst64, abs(p64 - 1.0)), max(worst32, abs(p32 - 1.0))
    print(f"order {order}: {len(contexts)} contexts, |sum - 1| <= {worst64:.2e} (float64), {worst32:.2e} (float32 table)")
    assert worst64 <= 1e-12 and worst32 <= 1e-5


def test_train_value_errors_and_save_load(tmp_path):
    for kw in (dict(order=0), dict(order=7), dict(discount=0.0), dict(discount=1.0)):
        with pytest.raises(ValueError):
            LM.CharLM.train(["ab"], **kw)
    with pytest.raises(ValueError):
        LM.train_ngrams([[1, 0, 2]], 2, 4)                               # the blank inside a line
    m = LM.CharLM.train(LR.synthetic_lines(8, 50), order=3)
    m.save(tmp_path / "lm.npz")
    with np.load(tmp_path / "lm.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["bo", "gram_ids", "gram_lens", "lp", "meta", "unk_lp"]
    back = LM.CharLM.load(tmp_path / "lm.npz")
    assert back.blob == m.blob and (back.order, back.num_classes, back.blank_id, back.unk_lp) == (3, 232, 0, m.unk_lp)
    assert back.score("tổng cộng") == m.score("tổng cộng") and back.score("tổng cộng", per_char=True)[1] == m.score("tổng cộng", True)[1]
    assert m.score([]) == 0.0 and m.score("") == 0.0


# ---------------------------------------------------------------------------------------------------- the search's definition
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("brute")])
def test_beam_lm_equals_brute_force_when_nothing_is_pruned(name):
    _, y, blank, W, _, tname, alpha, beta = LC.BY_NAME[name]
    want = LR.brute_lm(y[:, 0], blank, LC.table(tname), alpha, beta)
    got = LC.reference(name)[0][0]
    assert len(want) == {5: 25, 6: 41}[y.shape[0]] and len(want) < W and sorted(h[0] for h in got) == sorted(want)
    for l, R, s, g in got:
        assert abs(R - want[l][0]) <= 1e-13 * abs(want[l][0]) and abs(s - want[l][1]) <= 1e-14 * abs(want[l][1]) and _bits(g) == _bits(want[l][2])
    assert got[0][0] == max(want, key=lambda l: want[l][0])


def test_hand_made_rows():
    assert LC.reference("decide_a0")[0][0][0][0] == (1, 1)                # the acoustic scores alone
    assert LC.reference("decide_a1")[0][0][0][0] == (2, 2) and LC.reference("decide_a1")[0][0][0][3] == -0.5
    y = LC.BY_NAME["decide_a0"][1][:, 0]
    assert abs(y[0, 1] - y[0, 2]) < 1e-3 and abs(y[2, 1] - y[2, 2]) < 1e-3 and y[0, 1] > y[0, 2] and y[2, 1] > y[2, 2]
    assert [(h[0], h[1]) for h in LC.reference("tie_R_equal")[0][0]] == [((), -1.0), ((0,), -2.0), ((1,), -2.0), ((2,), -2.0)]
    assert [h[0] for h in LC.reference("tie_R_equal_W8")[0][0]] == [(), (0,), (1,), (2,), (4,), (5,), (6,), (7,)]
    assert [(h[0], h[1]) for h in LC.reference("tie_assoc")[0][0]] == [((2,), 2.0 ** 53), ((6,), 2.0 ** 53)]
    assert [h[0] for h in LC.reference("tie_assoc", "assoc")[0][0]] == [(6,), (2,)]
    assert [h[0] for h in LC.reference("one_hot_lm")[0][0]] == [(2, 3)] and LC.reference("dead_step_lm")[0][0] == []


def test_alpha_beta_zero_is_the_acoustic_search():
    """R = (s + 0 g) + 0 len is s exactly and the tie rule is shared: the reference with any table equals tests/ctcbeam_ref.py's."""
    import ctcbeam_cases as CC
    import ctcbeam_ref as BR
    for name, tname in (("identity_seed308_W4", "rand4_o3"), ("tie_blank0", "tie8"), ("nan_holes", "rand5_o3"), ("T64_C40_W16", "rand40_o3")):
        _, y, blank, W, _ = CC.BY_NAME[name]
        t = LC.table(tname) if tname != "tie8" or blank == 3 else LR.Table([((c,), -0.5 * c, 0.0) for c in range(1, 8)], 1, 8, 0, -3.0)
        got = LR.beam_lm(y[:, 0], blank, W, t, 0.0, 0.0)
        assert [(h[0], h[1]) for h in got] == BR.beam(y[:, 0], blank, W) and all(h[1] == h[2] for h in got)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in LC.EXACT])
def test_separation_condition(name):
    """tests/test_ctcbeam_cpu.py's condition on the rank totals: the smallest gap between consecutive R among the first W+1 candidates of
    any step, and between consecutive returned scores, is at least 1e-9 max(1, |R|).  Asserted, not filtered; ``ctclm_cases.EXACT`` is
    exempt by construction (exact ties, or at most one finite candidate)."""
    rows, gaps = LC.reference(name)
    nbest = LC.BY_NAME[name][4]
    smallest = np.inf
    for row, steps in zip(rows, gaps):
        for head, diff in steps:
            if len(diff):
                smallest = min(smallest, float((diff / np.maximum(1.0, np.abs(head[:-1]))).min()))
        sc = np.array([h[1] for h in row[:nbest]])
        if len(sc) > 1:
            smallest = min(smallest, float(((sc[:-1] - sc[1:]) / np.maximum(1.0, np.abs(sc[:-1]))).min()))
    print(f"{name}: smallest relative gap {smallest:.2e}")
    assert smallest >= 1e-9, (name, smallest)


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(LR.MUTANTS) and all(n in LC.BY_NAME for v in MUTANT_CASES.values() for n in v)


@pytest.mark.parametrize("mutant,name", [(m, n) for m, v in MUTANT_CASES.items() for n in v])
def test_each_mutant_changes_a_named_case(mutant, name):
    good, bad = LC.expected(name), LC.expected(name, mutant)
    ids_differ = not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    score_differs = False
    for a, b in zip(good[2:], bad[2:]):
        with np.errstate(invalid="ignore"):
            rel = np.abs(a - b) / np.maximum(1.0, np.abs(a))
        score_differs = score_differs or bool((np.nan_to_num(rel, nan=0.0, posinf=1.0) > 1e-6).any())
    assert ids_differ or score_differs, (mutant, name)


# ---------------------------------------------------------------------------------------------------- the C ABI's text, the Python layer
def test_exports_header_and_abi():
    header = open(os.path.join(ROOT, "include", "ocrvi.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"^(int|void) %s\(" % name, header, re.M), name
    for text in ("Character n-gram language model", "CTC prefix beam search with LM fusion", "#define OCRVI_LM_MAX_ORDER 6",
                 "(k << 60) | sum_j g_j << (10 (j-1))", "0x9e3779b97f4a7c15", "R = (s + alpha * g) + beta * len", "no end-of-line"):
        assert text in header.replace("There is no end-of-line", "no end-of-line"), text
    assert _lib.LM_MAX_ORDER == 6
    util = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "host_util.hip")).read()
    assert _lib.ABI_VERSION == 5 and "int ocrvi_abi_version(void) { return 5; }" in util
    src = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "ctc_beam_lm.hip")).read()
    for name in NEW_EXPORTS:
        assert re.search(r'extern "C" (int|void) %s\(' % name, src), name
    table_h = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "lm_table.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', table_h)      # a stand-alone program compiles against it: no HIP, no libocrvi header
    assert includes and not any("hip" in i or i.endswith("common.h") or i.endswith("ocrvi.h") for i in includes) and "__device__" not in table_h
    mk = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "Makefile")).read()
    assert "ctc_beam_lm.hip" in mk and "lm_table.h" in mk
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_EXPORTS) and lib.ocrvi_abi_version() == 5


def test_workspace_bytes_on_the_host():
    lib = _lib.load()
    n, m = C.c_size_t(7), C.c_size_t(0)
    for T, B, Cn, W in ((80, 256, 232, 8), (5, 1, 3, 32), (300, 2, 8, 64)):
        assert lib.ocrvi_ctc_beam_lm_workspace_bytes(T, B, Cn, W, C.byref(n)) == 0 and lib.ocrvi_ctc_beam_workspace_bytes(T, B, Cn, W, C.byref(m)) == 0
        rows = B * W * Cn * 8
        assert n.value == m.value + (rows + 255) // 256 * 256            # the prefixes, then [B][W][C] float64
    for T, B, Cn, W in ((0, 1, 3, 4), (1025, 1, 3, 4), (5, 0, 3, 4), (5, 1, 1, 4), (5, 1, 1025, 4), (5, 1, 3, 0), (5, 1, 3, 65)):
        n.value = 7
        assert lib.ocrvi_ctc_beam_lm_workspace_bytes(T, B, Cn, W, C.byref(n)) == EINVAL and n.value == 7
    assert lib.ocrvi_ctc_beam_lm_workspace_bytes(5, 1, 3, 4, None) == EINVAL


def test_check_lm_and_from_ngrams_raise_before_any_device_work():
    from ocr_vi_invoice_amd.rec import LMHypothesis, check_lm, make_lm_hypotheses
    m = LM.CharLM.from_ngrams({(1,): (-1.0, 0.0), (2,): (-2.0, 0.0)}, 1, 232)
    check_lm(None, 1.0, 0.0, None)
    check_lm(m, 0.0, -1.5, 4, 232, 0)
    bad = [(m, 1.0, 0.0, None), (None, 0.5, 0.0, 4), (None, 1.0, 0.1, None), (m, -0.1, 0.0, 4), (m, math.nan, 0.0, 4), (m, 1.0, math.inf, 4),
           (m, "1", 0.0, 4), ("table", 1.0, 0.0, 4), (m, 1.0, 0.0, 4, 231, 0), (m, 1.0, 0.0, 4, 232, 1)]
    for args in bad:
        with pytest.raises(ValueError):
            check_lm(*args)
    for grams, order in (({(1, 1): (-1.0, 0.0)}, 1), ({(1, 0): (-1.0, 0.0)}, 2), ({(0,): (-1.0, 0.0)}, 2), ({(400,): (-1.0, 0.0)}, 1),
                         ({(1,): (math.nan, 0.0)}, 1), ([((1,), -1.0, 0.0), ((1,), -2.0, 0.0)], 1), ({(1,): (-1.0, 0.0)}, 7)):
        with pytest.raises(ValueError):
            LM.CharLM.from_ngrams(grams, order, 232)
    with pytest.raises(ValueError):
        m.handle("cpu")
    assert m.score([1, 2, 3], per_char=True) == (-3.0 - math.log(231), [-1.0, -2.0, -math.log(231)])
    tok = LC.TOK
    a, b = sorted(tok.id_to_token)[:2]
    ids = np.full((1, 2, 4), -1, np.int32)
    ids[0, 0, :2] = (a, b)
    got = make_lm_hypotheses(tok, ids, np.array([[2, -1]], np.int32), np.array([[-1.5, -np.inf]]), np.array([[-0.5, -np.inf]]), np.array([[-2.0, -np.inf]]))
    assert got == [[LMHypothesis(tok.id_to_token[a] + tok.id_to_token[b], -1.5, (a, b), -0.5, -2.0)]]
