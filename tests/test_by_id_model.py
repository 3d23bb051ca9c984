"""The numpy model of the rows-by-id layer (tests/by_id_model.py) on hand cases: drop_self, the rule between the two directory
forms at its boundary, and the hash table against a plain dict on ids chosen to collide.  No GPU, no library."""
import numpy as np

from tests import by_id_model as bm

NAN = np.float32(np.nan)
PAD = bm.ABSENT


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def run(dist, ids, cnt, self_id, found=None):
    d, i = bm.drop_self(np.array([dist], dtype=np.float32), np.array([ids], dtype=np.uint32), [cnt], [self_id],
                        None if found is None else [found])
    return d[0], i[0]


def test_drop_self_hand_cases():
    # self first
    d, i = run([0.0, 1.0, 2.0, 3.0], [7, 4, 9, 2], 4, 7)
    assert same(d, [1.0, 2.0, 3.0]) and list(i) == [4, 9, 2]
    # self in the middle: the order of the others stays
    d, i = run([1.0, 0.5, 0.0, 3.0], [4, 9, 7, 2], 4, 7)
    assert same(d, [1.0, 0.5, 3.0]) and list(i) == [4, 9, 2]
    # self absent from its own result: the last entry leaves
    d, i = run([1.0, 0.5, 2.0, 3.0], [4, 9, 5, 2], 4, 7)
    assert same(d, [1.0, 0.5, 2.0]) and list(i) == [4, 9, 5]
    # a short row with self: two entries stay, one slot of padding
    d, i = run([0.0, 1.0, 2.0, 99.0], [7, 4, 9, 1234], 3, 7)
    assert same(d, [1.0, 2.0, NAN]) and list(i) == [4, 9, PAD]
    # a short row without self: its last VALID entry leaves, whatever lies behind the count
    d, i = run([1.0, 2.0, 99.0, 99.0], [4, 9, 7, 7], 2, 7)
    assert same(d, [1.0, NAN, NAN]) and list(i) == [4, PAD, PAD]
    # an empty row, and a row whose id has no stored row
    d, i = run([9.0, 9.0, 9.0, 9.0], [1, 2, 3, 4], 0, 7)
    assert same(d, [NAN] * 3) and list(i) == [PAD] * 3
    d, i = run([0.0, 1.0, 2.0, 3.0], [7, 4, 9, 2], 4, 7, found=False)
    assert same(d, [NAN] * 3) and list(i) == [PAD] * 3
    # a duplicate distance beside self (a bitwise-equal row with a smaller id comes first): only the entry with self's id leaves
    d, i = run([0.0, 0.0, 2.0, 3.0], [3, 7, 9, 2], 4, 7)
    assert same(d, [0.0, 2.0, 3.0]) and list(i) == [3, 9, 2]
    # self listed twice cannot happen (ids are unique), but "the first" is what the rule says
    d, i = run([0.0, 0.0, 2.0, 3.0], [7, 7, 9, 2], 4, 7)
    assert same(d, [0.0, 2.0, 3.0]) and list(i) == [7, 9, 2]


def test_form_rule_at_its_boundary():
    for n in (0, 1, 6000, 10 ** 8):
        edge = 4 * n + 65536
        assert bm.is_dense(edge, n) and not bm.is_dense(edge + 1, n)
        assert bm.is_dense(0, n) and bm.is_dense(n, n)
    assert not bm.is_dense(1 << 32, 6000)
    # the capacity: the power of two >= 2 n, at least 16
    assert [bm.hash_bits(n) for n in (0, 1, 8, 9, 6000, 8192, 8193)] == [4, 4, 4, 5, 14, 14, 15]
    for n in (1, 100, 6000, 6003, 1 << 20):
        cap = 1 << bm.hash_bits(n)
        assert cap >= 2 * n and (cap == 16 or cap // 2 < 2 * n)


def test_hash_is_the_documented_one():
    # home(id) = ((id * 0x9E3779B1) mod 2^32) >> (32 - bits), on values worked by hand
    assert bm.HASH_MUL == 0x9E3779B1
    assert list(bm.home([0, 1, 2, 0xFFFFFFFF], 4)) == [0, 0x9E3779B1 >> 28, ((2 * 0x9E3779B1) & 0xFFFFFFFF) >> 28,
                                                      ((0xFFFFFFFF * 0x9E3779B1) & 0xFFFFFFFF) >> 28]
    assert list(bm.home([12345], 14)) == [((12345 * 0x9E3779B1) & 0xFFFFFFFF) >> 18]


def test_table_against_a_dict_on_colliding_ids():
    rng = np.random.default_rng(5)
    n0 = 40
    bits = bm.hash_bits(n0 + 9)
    cap = 1 << bits
    base = rng.choice(1 << 20, size=n0, replace=False).astype(np.uint32)
    # four ids that share one home slot, and five that share the LAST slot: that run wraps past the table's end
    a = bm.colliding_ids(bits, 17, 4, lo=1 << 24, taken=base)
    b = bm.colliding_ids(bits, cap - 1, 5, lo=1 << 28, taken=np.concatenate([base, a]))
    assert set(bm.home(a, bits)) == {17} and set(bm.home(b, bits)) == {cap - 1}
    map_ids = np.concatenate([base, a, b])
    map_ids = map_ids[rng.permutation(len(map_ids))]
    slots, chain = bm.build_table(map_ids, bits)
    assert bits == bm.hash_bits(len(map_ids))
    want = {int(i): p for p, i in enumerate(map_ids)}
    # every stored id, ids that are not stored (some of them colliding with the runs), ids beyond every stored one
    miss = np.concatenate([bm.colliding_ids(bits, 17, 3, lo=1 << 30, taken=map_ids), bm.colliding_ids(bits, cap - 1, 3, lo=1 << 31, taken=map_ids),
                           rng.integers(0, 1 << 32, size=50, dtype=np.uint64).astype(np.uint32)])
    miss = miss[~np.isin(miss, map_ids)]
    ask = np.concatenate([map_ids, miss, map_ids[:5]])
    got = bm.table_lookup(slots, ask)
    assert [int(g) for g in got] == [want.get(int(i), bm.ABSENT) for i in ask]
    assert np.array_equal(got, bm.locate(map_ids, ask))
    # the occupied set: n slots, and the run of the last slot continues at slot 0
    occupied = np.nonzero(slots != np.uint64(bm.EMPTY))[0]
    assert len(occupied) == len(map_ids)
    at = {int(v) >> 32: s for s, v in enumerate(slots.tolist()) if v != bm.EMPTY}
    wrapped = [at[int(i)] for i in b if at[int(i)] != cap - 1]
    assert slots[cap - 1] != np.uint64(bm.EMPTY) and slots[0] != np.uint64(bm.EMPTY)
    assert len(wrapped) >= 4 and max(wrapped) < cap // 2         # at most one of the five sits in the last slot: the others wrapped
    # chains: t ids on one home slot give a chain of at least t, whatever the order
    assert chain[np.isin(map_ids, a)].max() >= 4 and chain[np.isin(map_ids, b)].max() >= 5
    assert chain.min() == 1
    # another insertion order: the same occupied set and the same answers
    perm = rng.permutation(len(map_ids))
    slots2, _ = bm.build_table(map_ids[perm], bits)
    assert np.array_equal(np.nonzero(slots2 != np.uint64(bm.EMPTY))[0], occupied)
    assert np.array_equal(perm[bm.table_lookup(slots2, map_ids)], np.arange(len(map_ids)))


def test_locate_model():
    map_ids = np.array([5, 0, 9, 2], dtype=np.uint32)
    assert list(bm.locate(map_ids, [9, 5, 5, 3, 0xFFFFFFFF, 0])) == [2, 0, 0, bm.ABSENT, bm.ABSENT, 1]
    assert list(bm.locate(map_ids, [9, 5, 2], live=[True, True, False, True])) == [bm.ABSENT, 0, 3]
    assert list(bm.locate(np.zeros(0, dtype=np.uint32), [1, 2])) == [bm.ABSENT, bm.ABSENT]
    assert bm.locate(map_ids, np.zeros(0, dtype=np.uint32)).shape == (0,)
