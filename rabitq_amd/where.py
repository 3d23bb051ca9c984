"""Predicates over attribute columns, as expressions: `col("ts") >= 5`, `.between(a, b)`, `.isin(values)`, `.any_bits(m)`,
`.all_bits(m)`, combined with `& | ~`.  `compile_expr` turns one into what rq_filter_create_where takes: a term table (column names
still -- RaBitQ.where resolves them to the index's columns and packs the constants in each column's type) and a postfix program.
Pure Python: nothing here touches the library or a GPU."""
from __future__ import annotations

OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_BETWEEN, OP_IN, OP_ANY_BITS, OP_ALL_BITS = range(10)   # RQ_WHERE_*
OP_NAMES = ("eq", "ne", "lt", "le", "gt", "ge", "between", "in", "any_bits", "all_bits")
TOK_AND, TOK_OR, TOK_NOT = 0x80, 0x81, 0x82                                                          # RQ_WHERE_AND / _OR / _NOT
MAX_TERMS, MAX_TOKENS, MAX_DEPTH, MAX_COLUMNS, MAX_SET = 32, 64, 32, 8, 4096


class Expr:
    """A boolean expression over columns.  Combine with & | ~ (Python's `and` / `or` / `not` cannot be overloaded and raise)."""

    def __and__(self, other):
        return And(self, _expr(other))

    def __or__(self, other):
        return Or(self, _expr(other))

    def __invert__(self):
        return Not(self)

    def __bool__(self):
        raise TypeError("a column predicate has no truth value: combine predicates with & | ~, and parenthesise comparisons")


def _expr(e):
    if not isinstance(e, Expr):
        raise TypeError(f"expected a column predicate, not {type(e).__name__}")
    return e


class Term(Expr):
    """One comparison of a column with constants: (column name, op, a, b, values)."""

    def __init__(self, column: str, op: int, a=0, b=0, values=()):
        self.column, self.op, self.a, self.b, self.values = column, op, a, b, tuple(values)

    def key(self):
        return (self.column, self.op, repr(self.a), repr(self.b), tuple(repr(v) for v in self.values))

    def __repr__(self):
        arg = {OP_BETWEEN: f"{self.a!r}, {self.b!r}", OP_IN: f"{list(self.values)!r}"}.get(self.op, f"{self.a!r}")
        return f'col("{self.column}").{OP_NAMES[self.op]}({arg})'


class And(Expr):
    def __init__(self, left, right):
        self.left, self.right = left, right

    def __repr__(self):
        return f"({self.left!r} & {self.right!r})"


class Or(Expr):
    def __init__(self, left, right):
        self.left, self.right = left, right

    def __repr__(self):
        return f"({self.left!r} | {self.right!r})"


class Not(Expr):
    def __init__(self, inner):
        self.inner = inner

    def __repr__(self):
        return f"~{self.inner!r}"


class Col:
    """A column by name; comparing it gives a Term."""

    __hash__ = None

    def __init__(self, name: str):
        if not isinstance(name, str):
            raise TypeError("a column is named by a string")
        self.name = name

    def __eq__(self, v):
        return Term(self.name, OP_EQ, v)

    def __ne__(self, v):
        return Term(self.name, OP_NE, v)

    def __lt__(self, v):
        return Term(self.name, OP_LT, v)

    def __le__(self, v):
        return Term(self.name, OP_LE, v)

    def __gt__(self, v):
        return Term(self.name, OP_GT, v)

    def __ge__(self, v):
        return Term(self.name, OP_GE, v)

    def between(self, a, b):
        """a <= value <= b"""
        return Term(self.name, OP_BETWEEN, a, b)

    def isin(self, values):
        """value == v for one of `values` (at most 4096)"""
        vals = tuple(values)
        if len(vals) > MAX_SET:
            raise ValueError(f"a set holds at most {MAX_SET} values")
        return Term(self.name, OP_IN, values=vals)

    def any_bits(self, mask):
        """(value & mask) != 0 -- integer columns"""
        return Term(self.name, OP_ANY_BITS, mask)

    def all_bits(self, mask):
        """(value & mask) == mask -- integer columns"""
        return Term(self.name, OP_ALL_BITS, mask)


def col(name: str) -> Col:
    return Col(name)


def compile_expr(expr):
    """-> (terms, program): terms a list of Term (equal terms appear once), program a list of tokens in postfix order -- an int below
    32 pushes that term, TOK_AND / TOK_OR pop two and push one, TOK_NOT negates the top.  Raises ValueError past the library's limits
    (32 terms, 64 tokens, stack depth 32, 8 distinct columns)."""
    terms, index, program = [], {}, []

    def emit(e):   # -> stack depth the sub-expression needs
        if isinstance(e, Term):
            k = e.key()
            if k not in index:
                index[k] = len(terms)
                terms.append(e)
            program.append(index[k])
            return 1
        if isinstance(e, Not):
            d = emit(e.inner)
            program.append(TOK_NOT)
            return d
        if isinstance(e, (And, Or)):
            dl = emit(e.left)
            dr = emit(e.right)
            program.append(TOK_AND if isinstance(e, And) else TOK_OR)
            return max(dl, 1 + dr)
        raise TypeError(f"expected a column predicate, not {type(e).__name__}")

    depth = emit(_expr(expr))
    if len(terms) > MAX_TERMS:
        raise ValueError(f"a predicate has at most {MAX_TERMS} distinct terms, not {len(terms)}")
    if len(program) > MAX_TOKENS:
        raise ValueError(f"a predicate's program has at most {MAX_TOKENS} tokens, not {len(program)}")
    if depth > MAX_DEPTH:
        raise ValueError(f"a predicate's program needs stack depth {depth}, more than {MAX_DEPTH}")
    if len({t.column for t in terms}) > MAX_COLUMNS:
        raise ValueError(f"a predicate reads at most {MAX_COLUMNS} distinct columns")
    return terms, program
