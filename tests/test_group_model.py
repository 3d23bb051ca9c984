"""The model of grouped search (tests/group_model.py) on cases worked by hand, and its two forms of the selection against each
other on random inputs.  No GPU needed."""
import numpy as np

from tests import group_model as M

NAN = M.PAD_DIST_BITS
PAD = M.PAD_ID


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def run(dist, ids, keymap, topk, g, cnt=None, select=M.select_by_walk):
    dist = np.asarray([dist], dtype=np.float32)
    ids = np.asarray([ids], dtype=np.uint32)
    return M.group_rows(dist, ids, [len(dist[0]) if cnt is None else cnt], keymap, topk, g, select)


def both(dist, ids, keymap, topk, g, cnt=None):
    a, b = run(dist, ids, keymap, topk, g, cnt, M.select_by_walk), run(dist, ids, keymap, topk, g, cnt, M.select_by_rank)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    return a


def test_ord32_biased_orders_floats_as_the_library_does():
    v = np.array([-np.inf, -2.5, -0.0, 0.0, 1e-30, 1.0, np.inf], dtype=np.float32)
    k = M.ord32_biased(v)
    assert list(k) == sorted(k) and len(set(k.tolist())) == len(v)            # -0 below +0: bit patterns, not values
    assert M.ord32_biased(np.float32(0.0)) == 0x80000000


def test_hand_case_two_per_group():
    # distance order: id 5 (A), 9 (B), 2 (A), 7 (A), 4 (C), 1 (B); given shuffled
    keymap = {5: 10, 9: 20, 2: 10, 7: 10, 4: 30, 1: 20}
    out = both([0.5, 0.1, 0.6, 0.2, 0.3, 0.4], [4, 5, 1, 9, 2, 7], keymap, 2, 2)
    assert out["ids"].tolist() == [[[5, 2], [9, 1]]]                          # A first (nearest row), two of its three rows
    assert out["dist_bits"].tolist() == [[bits([0.1, 0.3]).tolist(), bits([0.2, 0.6]).tolist()]]
    assert out["keys"].tolist() == [[10, 20]] and out["group_n"].tolist() == [[2, 2]] and out["n"].tolist() == [2]
    assert (out["absent"], out["kept"], out["groups"]) == (0, 4, 2)


def test_all_ties_are_decided_by_id():
    keymap = {i: i % 2 for i in range(6)}
    out = both([1.0] * 6, [5, 3, 4, 0, 2, 1], keymap, 2, 2)
    assert out["ids"].tolist() == [[[0, 2], [1, 3]]] and out["keys"].tolist() == [[0, 1]]


def test_one_group_and_padding():
    keymap = {i: 7 for i in range(5)}
    out = both([0.3, 0.1, 0.2, 0.5, 0.4], [0, 1, 2, 3, 4], keymap, 3, 2)
    assert out["ids"].tolist() == [[[1, 2], [PAD, PAD], [PAD, PAD]]]
    assert out["dist_bits"][0, 1:].tolist() == [[NAN, NAN], [NAN, NAN]]
    assert out["keys"].tolist() == [[7, 0, 0]] and out["group_n"].tolist() == [[2, 0, 0]] and out["n"].tolist() == [1]


def test_all_distinct():
    keymap = {i: 100 + i for i in range(5)}
    out = both([0.5, 0.4, 0.3, 0.2, 0.1], [0, 1, 2, 3, 4], keymap, 3, 2)
    assert out["ids"].tolist() == [[[4, PAD], [3, PAD], [2, PAD]]]
    assert out["keys"].tolist() == [[104, 103, 102]] and out["group_n"].tolist() == [[1, 1, 1]] and out["n"].tolist() == [3]


def test_no_candidate():
    out = both([0.5, 0.4], [0, 1], {0: 1, 1: 2}, 2, 2, cnt=0)
    assert (out["ids"] == PAD).all() and (out["dist_bits"] == NAN).all() and not out["keys"].any() and not out["group_n"].any()
    assert out["n"].tolist() == [0] and (out["absent"], out["kept"], out["groups"]) == (0, 0, 0)


def test_entries_past_cnt_are_not_read():
    out = both([0.5, 0.4, 0.0], [0, 1, 2], {0: 1, 1: 2, 2: 3}, 3, 1, cnt=2)
    assert out["ids"].tolist() == [[[1], [0], [PAD]]]


def test_an_absent_id_is_skipped_and_counted():
    keymap = {1: 5, 2: 6}                                                     # id 9 has no live row
    out = both([0.1, 0.2, 0.3], [9, 1, 2], keymap, 2, 1)
    assert out["ids"].tolist() == [[[1], [2]]] and out["absent"] == 1 and out["kept"] == 2
    out = both([0.1], [9], keymap, 1, 1)                                      # ... and opens no group
    assert out["n"].tolist() == [0] and out["absent"] == 1


def test_u64_keys_that_differ_in_the_high_word_only():
    keymap = {0: 7, 1: (1 << 32) | 7, 2: 7, 3: (2 << 32) | 7}
    out = both([0.1, 0.2, 0.3, 0.4], [0, 1, 2, 3], keymap, 3, 2)
    assert out["ids"].tolist() == [[[0, 2], [1, PAD], [3, PAD]]]
    assert out["keys"].tolist() == [[7, (1 << 32) | 7, (2 << 32) | 7]]


def test_key_images():
    assert M.key_image(np.array([-1, 2], dtype=np.int32)).tolist() == [0xFFFFFFFF, 2]          # zero-extended, not sign-extended
    assert M.key_image(np.array([-1], dtype=np.int64)).tolist() == [0xFFFFFFFFFFFFFFFF]
    assert M.key_image(np.array([1 << 40], dtype=np.uint64)).tolist() == [1 << 40]
    assert M.keymap_of([4, 9], np.array([-1, 3], dtype=np.int32), live=[True, False]) == {4: 0xFFFFFFFF}


def test_the_two_forms_agree_on_random_inputs():
    rng = np.random.default_rng(11)
    for trial in range(60):
        F = int(rng.integers(1, 40))
        B = 3
        nkeys = int(rng.integers(1, 8))
        ids = np.stack([rng.permutation(64)[:F] for _ in range(B)]).astype(np.uint32)
        dist = rng.integers(0, 5, size=(B, F)).astype(np.float32) / 4           # many ties
        cnt = rng.integers(0, F + 1, size=B)
        keymap = {i: int(rng.integers(0, nkeys)) << int(rng.integers(0, 2) * 32) for i in range(64) if rng.random() > 0.1}
        topk, g = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        a = M.group_rows(dist, ids, cnt, keymap, topk, g, M.select_by_walk)
        b = M.group_rows(dist, ids, cnt, keymap, topk, g, M.select_by_rank)
        for name in a:
            assert np.array_equal(a[name], b[name]), (trial, name)
        # any order of the pairs inside a row gives the same answer
        perm = [rng.permutation(int(cnt[r])) for r in range(B)]
        d2, i2 = dist.copy(), ids.copy()
        for r in range(B):
            d2[r, :cnt[r]], i2[r, :cnt[r]] = dist[r, perm[r]], ids[r, perm[r]]
        c = M.group_rows(d2, i2, cnt, keymap, topk, g, M.select_by_walk)
        for name in a:
            assert np.array_equal(a[name], c[name]), (trial, name, "shuffled")
