"""tests/merge_model.py (the ranks-and-counts model of merge_lists_kernel) against a plain sort of the union's 64-bit keys: random
lists with empty lists on either side, equal key words whose order the ids decide, an empty side; and the extract map against
boolean indexing."""
import numpy as np
import pytest

from tests import merge_model as mm


def random_index(rng, k, max_len, empty_every, id_pool, words_from):
    """k lists of random length (every `empty_every`-th empty), each ascending by (key word, id); key words drawn from the small
    set `words_from`, so that many rows share a word and the id decides."""
    lens = rng.integers(0, max_len + 1, size=k)
    if empty_every:
        lens[::empty_every] = 0
    off = np.zeros(k + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    ids = rng.permutation(id_pool)[:n].astype(np.uint32)
    words = rng.choice(words_from, size=n).astype(np.uint32)
    for c in range(k):
        s = slice(off[c], off[c + 1])
        order = np.argsort(mm.keys64(words[s], ids[s]), kind="stable")
        words[s], ids[s] = words[s][order], ids[s][order]
    return off, words, ids


def by_sorting(off_a, words_a, ids_a, off_b, words_b, ids_b, shift):
    k, n_a = off_a.size - 1, int(off_a[-1])
    ka, kb = mm.keys64(words_a, ids_a), mm.keys64(words_b, ids_b, shift)
    out_off, parts = [0], []
    for c in range(k):
        keys = np.concatenate([ka[off_a[c]:off_a[c + 1]], kb[off_b[c]:off_b[c + 1]]])
        src = np.concatenate([np.arange(off_a[c], off_a[c + 1]), n_a + np.arange(off_b[c], off_b[c + 1])])
        assert np.unique(keys).size == keys.size
        parts.append(src[np.argsort(keys, kind="stable")])
        out_off.append(out_off[-1] + keys.size)
    return np.array(out_off, dtype=np.uint32), np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("shift", [0, 1000, 0xFFFF0000])
def test_merge_map_equals_sort_of_the_union(seed, shift):
    rng = np.random.default_rng(seed)
    k = 13
    words_from = np.array([0, 1, 7, 7, 0x7F7FFFFF, 0xFFFFFFFF], dtype=np.uint32)   # few words: most keys tie on the word
    a = random_index(rng, k, 40, 3, np.arange(0, 2000, 2), words_from)             # even ids; lists 0, 3, 6 .. empty
    b = random_index(rng, k, 40, 4, np.arange(1, 2000, 2), words_from)             # odd ids + an even shift: clear of A's
    got = mm.merge_lists(*a, *b, shift=shift)
    want = by_sorting(*a, *b, shift)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(np.sort(got[1]), np.arange(got[1].size))                  # a permutation: no hole, nothing twice
    # the merged list ascends by key
    n_a = int(a[0][-1])
    allk = np.concatenate([mm.keys64(a[1], a[2]), mm.keys64(b[1], b[2], shift)])
    merged = allk[got[1]]
    for c in range(k):
        assert (np.diff(merged[got[0][c]:got[0][c + 1]].astype(object)) > 0).all()
    assert n_a + int(b[0][-1]) == got[1].size


def test_same_word_on_both_sides_the_id_decides_either_way():
    off = np.array([0, 2], dtype=np.uint32)
    wa, ia = np.array([5, 5], np.uint32), np.array([10, 20], np.uint32)
    wb, ib = np.array([5, 5], np.uint32), np.array([10, 20], np.uint32)
    _, before = mm.merge_lists(off, wa, ia, off, wb, ib, shift=5)      # B's copies sort after A's: 10 15 20 25
    assert before.tolist() == [0, 2, 1, 3]
    wa2, ia2 = np.array([5, 5], np.uint32), np.array([110, 120], np.uint32)
    _, after = mm.merge_lists(off, wa2, ia2, off, wb, ib, shift=0)     # B's sort before A's
    assert after.tolist() == [2, 3, 0, 1]


def test_an_empty_side_gives_the_other_back():
    rng = np.random.default_rng(9)
    a = random_index(rng, 5, 30, 2, np.arange(500), np.array([3, 4], np.uint32))
    empty = (np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    off, m = mm.merge_lists(*a, *empty)
    assert np.array_equal(off, a[0]) and np.array_equal(m, np.arange(a[2].size))
    off, m = mm.merge_lists(*empty, *a, shift=77)
    assert np.array_equal(off, a[0]) and np.array_equal(m, np.arange(a[2].size))    # n_a == 0: positions of B as they are


@pytest.mark.parametrize("seed", range(4))
def test_extract_map_equals_boolean_indexing(seed):
    rng = np.random.default_rng(100 + seed)
    off, words, ids = random_index(rng, 11, 50, 3, np.arange(3000), np.array([1, 2, 3], np.uint32))
    allowed = rng.random(2500) < (0.0 if seed == 0 else 0.4)           # ids >= 2500 are beyond the bitmap: not taken
    out_off, m = mm.extract_lists(off, ids, allowed)
    keep = (ids < allowed.size) & allowed[np.minimum(ids, allowed.size - 1)]
    assert np.array_equal(m, np.nonzero(keep)[0])
    lists = np.repeat(np.arange(11), np.diff(off.astype(np.int64)))
    assert np.array_equal(np.diff(out_off.astype(np.int64)), np.bincount(lists[keep], minlength=11))
    # the same map from the merge with an empty other side, on the kept rows alone
    sub_off = out_off
    empty = (np.zeros(12, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    off2, m2 = mm.merge_lists(sub_off, words[keep], ids[keep], *empty)
    assert np.array_equal(off2, sub_off) and np.array_equal(m2, np.arange(int(keep.sum())))
