"""A numpy model of the attribute columns (include/rabitq_hip.h, "attribute columns"): the typed comparisons of a predicate's terms,
the postfix evaluation of its program, and the bookkeeping of {id: value} per column through add, remove, merge and extract with
the fill rules of the header.  The GPU tests compare the library with it; tests/test_attr_model.py pins it to hand-written cases."""
import numpy as np

DTYPES = {"u32": np.uint32, "i32": np.int32, "f32": np.float32, "u64": np.uint64, "i64": np.int64}
EQ, NE, LT, LE, GT, GE, BETWEEN, IN, ANY_BITS, ALL_BITS = range(10)
TOK_AND, TOK_OR, TOK_NOT = 0x80, 0x81, 0x82


def const(dtype, v):
    """A constant in the column's type (the exact value, as the Python layer packs it)."""
    return np.array([v]).astype(DTYPES[dtype])[0] if dtype == "f32" else DTYPES[dtype](int(v))


def term(dtype, values, op, a=0, b=0, members=()):
    """The truth value of one term for every element of `values` (an array of the column's dtype): comparisons in the type's own
    order -- unsigned, signed, IEEE (a NaN fails everything but NE, -0 == +0) --, the bit ops on the unsigned image."""
    v = np.asarray(values, dtype=DTYPES[dtype])
    if op in (ANY_BITS, ALL_BITS):
        assert dtype != "f32", "the bit ops are for integer columns"
        u = np.uint32 if v.dtype.itemsize == 4 else np.uint64
        bits, mask = v.view(u), np.array([const(dtype, a)]).view(u)[0]
        return (bits & mask) != 0 if op == ANY_BITS else (bits & mask) == mask
    if op == IN:
        out = np.zeros(v.shape, dtype=bool)
        for m in members:                       # v == s for some s: == is the type's own (NaN equals nothing)
            out |= v == const(dtype, m)
        return out
    ca = const(dtype, a)
    with np.errstate(invalid="ignore"):
        if op == EQ:
            return v == ca
        if op == NE:
            return v != ca
        if op == LT:
            return v < ca
        if op == LE:
            return v <= ca
        if op == GT:
            return v > ca
        if op == GE:
            return v >= ca
        if op == BETWEEN:
            return (ca <= v) & (v <= const(dtype, b))
    raise ValueError(f"unknown op {op}")


def program_check(program, nterms):
    """What the library refuses: -> None, or the reason."""
    if len(program) > 64:
        return "more than 64 tokens"
    depth = 0
    for tok in program:
        if tok < 32:
            if tok >= nterms:
                return "a term that does not exist"
            depth += 1
            if depth > 32:
                return "deeper than 32"
        elif tok in (TOK_AND, TOK_OR):
            if depth < 2:
                return "underflow"
            depth -= 1
        elif tok == TOK_NOT:
            if depth < 1:
                return "underflow"
        else:
            return "unknown token"
    return None if depth == 1 else f"ends at depth {depth}"


def evaluate(program, truths, n):
    """The postfix program over the terms' truth arrays (truths[i]: term i for every row) -> the admitted rows (bool, n).  program
    None: the AND of all terms; no term at all: every row."""
    if program is None:
        out = np.ones(n, dtype=bool)
        for t in truths:
            out &= t
        return out
    assert program_check(program, len(truths)) is None
    stack = []
    for tok in program:
        if tok < 32:
            stack.append(np.asarray(truths[tok], dtype=bool))
        elif tok == TOK_AND:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b)
        elif tok == TOK_OR:
            b, a = stack.pop(), stack.pop()
            stack.append(a | b)
        else:
            stack.append(~stack.pop())
    return stack[0]


def where(columns, terms, program):
    """columns: {name: (dtype, values)}; terms: [(name, op, a, b, members)] -> the admitted rows (bool)."""
    n = len(next(iter(columns.values()))[1]) if columns else 0
    truths = [term(columns[name][0], columns[name][1], op, a, b, members) for name, op, a, b, members in terms]
    return evaluate(program, truths, n)


class Columns:
    """{id: value} per column of one index, moved along with the index's rows."""

    def __init__(self, ids=()):
        self.ids = set(int(i) for i in ids)
        self.cols = {}          # name -> [dtype, fill, {id: value}], in creation order

    def create(self, name, dtype, fill=0):
        assert name not in self.cols and len(self.cols) < 16
        f = const(dtype, fill)
        self.cols[name] = [dtype, f, {i: f for i in self.ids}]

    def drop(self, name):
        del self.cols[name]

    def set(self, name, ids, values):
        """-> absent ids (counted per occurrence); the last occurrence of an id wins"""
        dtype, _, vals = self.cols[name]
        absent = 0
        for i, v in zip(ids, values):
            if int(i) in self.ids:
                vals[int(i)] = const(dtype, v) if dtype != "f32" else np.float32(v)
            else:
                absent += 1
        return absent

    def get(self, name, ids):
        dtype, fill, vals = self.cols[name]
        out = np.array([vals.get(int(i), fill) for i in ids], dtype=DTYPES[dtype])
        return out, np.array([int(i) in self.ids for i in ids], dtype=bool)

    def array(self, name, map_ids):
        """the column in position order, given the index's map_ids"""
        dtype, _, vals = self.cols[name]
        return np.array([vals[int(i)] for i in map_ids], dtype=DTYPES[dtype])

    def add(self, ids):
        """new rows hold every column's fill"""
        for i in ids:
            assert int(i) not in self.ids
            self.ids.add(int(i))
            for _, fill, vals in self.cols.values():
                vals[int(i)] = fill

    def remove(self, ids):
        for i in ids:
            if int(i) in self.ids:
                self.ids.discard(int(i))
                for _, _, vals in self.cols.values():
                    del vals[int(i)]

    def merge_from(self, other, shift=0):
        """rows of `other` (ids + shift) bring its value where it has a column of the same name and type, else they hold this index's
        fill; the same name with another type is refused; columns only `other` has are not taken"""
        for name, (dtype, _, _) in self.cols.items():
            if name in other.cols and other.cols[name][0] != dtype:
                raise ValueError(f"column {name}: type clash")
        for i in other.ids:
            assert i + shift not in self.ids
        for i in other.ids:
            self.ids.add(i + shift)
            for name, (dtype, fill, vals) in self.cols.items():
                vals[i + shift] = other.cols[name][2][i] if name in other.cols else fill

    def extract(self, ids):
        """a new index's columns: every column, the rows of `ids` this index holds"""
        out = Columns(i for i in ids if int(i) in self.ids)
        for name, (dtype, fill, vals) in self.cols.items():
            out.cols[name] = [dtype, fill, {i: vals[i] for i in out.ids}]
        return out

    def copy(self):
        return self.extract(self.ids)
