"""tests/attr_model.py against hand-written cases, and the expression compiler of rabitq_amd/where.py against expected term and
token lists.  No GPU needed."""
import numpy as np
import pytest

from rabitq_amd import where as W
from rabitq_amd.where import col
from tests import attr_model as M

A, O, N = M.TOK_AND, M.TOK_OR, M.TOK_NOT


def bools(s):
    return np.array([c == "1" for c in s])


def test_f32_nan_and_signed_zero():
    v = np.array([np.nan, -0.0, 0.0, 1.5, -np.inf], dtype=np.float32)
    assert np.array_equal(M.term("f32", v, M.EQ, 0.0), bools("01100"))            # -0 == +0
    assert np.array_equal(M.term("f32", v, M.EQ, -0.0), bools("01100"))
    assert np.array_equal(M.term("f32", v, M.NE, 0.0), bools("10011"))            # a NaN passes NE ...
    for op in (M.EQ, M.LT, M.LE, M.GT, M.GE):                                     # ... and fails everything else
        assert not M.term("f32", v, op, 1.0)[0]
    assert not M.term("f32", v, M.BETWEEN, -np.inf, np.inf)[0]
    assert np.array_equal(M.term("f32", v, M.BETWEEN, -np.inf, np.inf), bools("01111"))
    assert not M.term("f32", v, M.EQ, np.nan).any()                               # a NaN constant: EQ holds nowhere, NE everywhere
    assert M.term("f32", v, M.NE, np.nan).all()
    assert np.array_equal(M.term("f32", v, M.IN, members=[np.nan, 0.0]), bools("01100"))
    assert np.array_equal(M.term("f32", v, M.LT, 0.0), bools("00001"))
    assert np.array_equal(M.term("f32", v, M.LE, -0.0), bools("01101"))


def test_signed_against_unsigned_images():
    bits = np.array([0xFFFFFFFF, 0, 1, 0x80000000], dtype=np.uint32)
    assert np.array_equal(M.term("u32", bits, M.GT, 1), bools("1001"))            # 0xFFFFFFFF is the largest u32 ...
    assert np.array_equal(M.term("i32", bits.view(np.int32), M.GT, 1), bools("0000"))   # ... and -1 as an i32
    assert np.array_equal(M.term("i32", bits.view(np.int32), M.LT, 0), bools("1001"))
    assert np.array_equal(M.term("i32", bits.view(np.int32), M.EQ, -1), bools("1000"))
    assert np.array_equal(M.term("u32", bits, M.EQ, 0xFFFFFFFF), bools("1000"))
    assert np.array_equal(M.term("i32", bits.view(np.int32), M.ANY_BITS, -2**31), bools("1001"))
    assert np.array_equal(M.term("u32", bits, M.ALL_BITS, 0x80000001), bools("1000"))
    assert np.array_equal(M.term("u32", bits, M.ALL_BITS, 0), bools("1111"))      # (v & 0) == 0
    assert np.array_equal(M.term("u32", bits, M.ANY_BITS, 0), bools("0000"))


def test_u64_above_2_32_and_i64():
    v = np.array([2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**64 - 1], dtype=np.uint64)
    assert np.array_equal(M.term("u64", v, M.GE, 2**32), bools("01111"))
    assert np.array_equal(M.term("u64", v, M.EQ, 2**32 + 1), bools("00100"))      # not its low word, 1
    assert np.array_equal(M.term("u64", v, M.EQ, 1), bools("00000"))
    assert np.array_equal(M.term("u64", v, M.BETWEEN, 2**32, 2**63), bools("01110"))
    assert np.array_equal(M.term("i64", v.view(np.int64), M.LT, 0), bools("00011"))
    assert np.array_equal(M.term("i64", v.view(np.int64), M.BETWEEN, -1, 2**32), bools("11001"))
    assert np.array_equal(M.term("u64", v, M.ANY_BITS, 2**32), bools("01101"))
    assert np.array_equal(M.term("u64", v, M.IN, members=[2**64 - 1, 2**32]), bools("01001"))


def test_empty_between_and_in_sizes():
    v = np.arange(10000, dtype=np.uint32)
    assert not M.term("u32", v, M.BETWEEN, 7, 6).any()                            # a > b: empty
    assert M.term("u32", v, M.BETWEEN, 7, 7).sum() == 1
    assert not M.term("u32", v, M.IN, members=[]).any()
    rng = np.random.default_rng(5)
    for count in (1, 17, 4096):
        members = rng.choice(20000, size=count, replace=False)
        got = M.term("u32", v, M.IN, members=members)
        assert np.array_equal(got, np.isin(v, members)) and got.sum() == (members < 10000).sum()


def test_programs_de_morgan_and_depth():
    rng = np.random.default_rng(9)
    n = 257
    t = [rng.random(n) < 0.5 for _ in range(3)]
    pairs = [([0, 1, A, N], [0, N, 1, N, O]), ([0, 1, O, N], [0, N, 1, N, A]),
             ([0, 1, A, 2, O, N], [0, N, 1, N, O, 2, N, A])]
    for left, right in pairs:
        assert np.array_equal(M.evaluate(left, t, n), M.evaluate(right, t, n))
    assert np.array_equal(M.evaluate([0, 1, A, N], t, n), ~(t[0] & t[1]))
    assert np.array_equal(M.evaluate(None, t, n), t[0] & t[1] & t[2])             # no program: the AND of all terms
    assert M.evaluate(None, [], n).all()                                          # no term: every row
    # a chain that needs depth 32: 32 pushes, then 31 ORs -- 63 tokens
    truths = [rng.random(n) < 0.05 for _ in range(32)]
    deep = list(range(32)) + [O] * 31
    assert M.program_check(deep, 32) is None
    assert np.array_equal(M.evaluate(deep, truths, n), np.logical_or.reduce(truths))
    # what the library refuses
    assert M.program_check([0, A], 1) == "underflow" and M.program_check([N], 1) == "underflow"
    assert M.program_check([0, 1], 2) == "ends at depth 2" and M.program_check([], 0) == "ends at depth 0"
    assert M.program_check([3], 3) == "a term that does not exist" and M.program_check([0, 0x83], 1) == "unknown token"
    assert M.program_check([0] * 33 + [A] * 32, 1) == "more than 64 tokens"
    assert M.program_check([0] * 33 + [A] * 31, 1) == "deeper than 32"


def test_column_bookkeeping():
    a = M.Columns(range(10))
    a.create("t", "u32", 7)
    a.create("w", "f32", 0.5)
    assert a.set("t", [1, 2, 99, 1], [10, 20, 30, 11]) == 1                       # 99 is absent; the last 1 wins
    v, f = a.get("t", [1, 2, 3, 99])
    assert v.tolist() == [11, 20, 7, 7] and f.tolist() == [True, True, True, False]
    a.add([20, 21])                                                               # new rows hold the fill
    assert a.get("t", [20])[0].tolist() == [7] and a.get("w", [21])[0].tolist() == [0.5]
    a.remove([2, 55])
    assert a.get("t", [2]) [1].tolist() == [False] and a.get("t", [2])[0].tolist() == [7]
    b = M.Columns([0, 1])
    b.create("t", "u32", 3)
    b.create("only_b", "i64", -1)
    b.set("t", [1], [100])
    a.merge_from(b, shift=100)
    assert a.get("t", [100, 101])[0].tolist() == [3, 100]                         # src's values, its fill included
    assert a.get("w", [100])[0].tolist() == [0.5] and "only_b" not in a.cols      # dst's fill; src-only columns are not taken
    c = M.Columns([5])
    c.create("t", "i32", 0)
    with pytest.raises(ValueError):
        a.merge_from(c, shift=1000)
    assert 1005 not in a.ids
    e = a.extract([1, 100, 77])
    assert e.ids == {1, 100} and list(e.cols) == ["t", "w"] and e.get("t", [1, 100])[0].tolist() == [11, 3]
    assert a.array("t", [101, 1, 0]).tolist() == [100, 11, 7]
    assert a.copy().cols["t"][2] == a.cols["t"][2]


def test_expression_compiler():
    terms, prog = W.compile_expr(col("ts") >= 5)
    assert [(t.column, t.op, t.a) for t in terms] == [("ts", W.OP_GE, 5)] and prog == [0]
    e = (col("tenant") == 7) & (col("ts") >= 5) & ~col("flags").any_bits(6)
    terms, prog = W.compile_expr(e)
    assert [(t.column, t.op, t.a) for t in terms] == [("tenant", W.OP_EQ, 7), ("ts", W.OP_GE, 5), ("flags", W.OP_ANY_BITS, 6)]
    assert prog == [0, 1, A, 2, N, A]
    e = col("a").between(1, 9) | (col("b").isin([3, 1, 2]) & (col("a") != 4)) | col("a").between(1, 9)
    terms, prog = W.compile_expr(e)                                               # the repeated term appears once
    assert [(t.column, t.op, t.a, t.b, t.values) for t in terms] == [
        ("a", W.OP_BETWEEN, 1, 9, ()), ("b", W.OP_IN, 0, 0, (3, 1, 2)), ("a", W.OP_NE, 4, 0, ())]
    assert prog == [0, 1, 2, A, O, 0, O]
    assert [t.op for t in W.compile_expr((col("x") < 1) | (col("x") <= 1) | (col("x") > 1) | col("x").all_bits(1))[0]] == [
        W.OP_LT, W.OP_LE, W.OP_GT, W.OP_ALL_BITS]
    assert (W.TOK_AND, W.TOK_OR, W.TOK_NOT) == (A, O, N) and W.OP_ALL_BITS == M.ALL_BITS == 9
    # the compiled program is one the model accepts and evaluates as Python would
    cols = {"a": ("u32", np.arange(20, dtype=np.uint32)), "b": ("i32", np.arange(20, dtype=np.int32) % 5)}
    got = M.where(cols, [(t.column, t.op, t.a, t.b, t.values) for t in terms], prog)
    a_, b_ = cols["a"][1], cols["b"][1]
    assert np.array_equal(got, ((a_ >= 1) & (a_ <= 9)) | (np.isin(b_, [1, 2, 3]) & (a_ != 4)))
    with pytest.raises(TypeError):
        bool(col("a") == 1)                                                       # `and` / `or` / chained comparisons
    with pytest.raises(TypeError):
        (col("a") == 1) & True
    with pytest.raises(ValueError):
        col("a").isin(range(4097))
    many = col("c0") == 0
    for i in range(1, 9):
        many = many & (col(f"c{i}") == 0)
    with pytest.raises(ValueError, match="8 distinct columns"):
        W.compile_expr(many)
    wide = col("a") == 0
    for i in range(1, 33):
        wide = wide | (col("a") == i)
    with pytest.raises(ValueError, match="32 distinct terms"):
        W.compile_expr(wide)
    right = col("a") == 32                                                        # right-nested: every level needs one more slot
    for i in range(31, -1, -1):
        right = (col("a") == (i % 30)) | right
    with pytest.raises(ValueError):
        W.compile_expr(right)
