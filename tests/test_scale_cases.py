"""tests/scale_cases.py against the sources: the launch sites of the bookkeeping kernels are parsed (no GPU) and the table must state
what they say, so that a changed grid cap fails here instead of silently un-covering a grid-stride loop; every count the GPU module
sends through a kernel must be past that kernel's first trip; and the vectorised models of scale_cases.py equal the per-row models
on small inputs."""
import os
import re

import numpy as np
import pytest

from tests import attr_model as AM
from tests import by_id_model as BM
from tests import group_model as GM
from tests import scale_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rabitq_amd", "csrc")
THREADS = 256
_SRC = {}


def source(name):
    if name not in _SRC:
        _SRC[name] = open(os.path.join(CSRC, name)).read()
    return _SRC[name]


def number(expr, names=None):
    """A grid expression's constant (`4096`, `1u << 16`, `4 * R`) as an int."""
    e = re.sub(r"\b(\d+)u(ll)?\b", r"\1", expr.strip())
    for k, v in (names or {}).items():
        e = re.sub(r"\b%s\b" % k, str(v), e)
    assert re.fullmatch(r"[\d\s*<()+]+", e), expr
    return int(eval(e))


def balanced(text, at):
    """text[at] == '(' -> the index past its closing parenthesis."""
    depth = 0
    for j in range(at, len(text)):
        depth += {"(": 1, ")": -1}.get(text[j], 0)
        if depth == 0:
            return j + 1
    raise AssertionError("unbalanced")


def launches(text, kernel):
    """-> [(grid expression, block expression, offset)] of every `kernel<...><<<grid, block...>>>` in text."""
    out = []
    for m in re.finditer(r"\b%s\b(?:<[^<>;()]*>)?<<<" % kernel, text):
        at, depth, parts, start = m.end(), 0, [], m.end()
        while not (depth == 0 and text.startswith(">>>", at)):
            c = text[at]
            depth += {"(": 1, ")": -1}.get(c, 0)
            if c == "<" and re.match(r"<\w+>\(", text[at:]):                   # min<uint64_t>( : a template argument, not a comparison
                at = text.index(">", at)
            elif c == "," and depth == 0:
                parts.append(text[start:at].strip())
                start = at + 1
            at += 1
        parts.append(text[start:at].strip())
        out.append((parts[0], parts[1], m.start()))
    return out


def named(text, offset, name):
    """The initialiser of the nearest `name = ...;` before offset (a grid kept in a local)."""
    found = list(re.finditer(r"\b%s = ([^;]+);" % name, text[:offset]))
    assert found, name
    return found[-1].group(1).strip()


MIN_GRID = re.compile(r"^\(uint32_t\)std::min<uint64_t>\(ceil_div\((.+), ([^,]+)\), ([^,]+)\)$")


def attr_grid_cap():
    m = re.search(r"static uint32_t attr_grid\(uint64_t count\) \{ return \(uint32_t\)std::max<uint64_t>\(1, std::min<uint64_t>\("
                  r"ceil_div\(count, (\d+)\), (\d+)\)\); \}", source("host_attr.h"))
    assert m, "attr_grid is not written as the table's parser knows it"
    assert int(m.group(1)) == THREADS
    return int(m.group(2))


def per_trip_of(case, kernel):
    """What the sources say one trip of `kernel`'s grid covers, in the items the table counts."""
    text = source(case["file"])
    sites = launches(text, kernel)
    assert sites, (kernel, "no launch in", case["file"])
    got = set()
    for grid, block, at in sites:
        assert block == str(THREADS), (kernel, block)
        if re.fullmatch(r"\w+", grid):
            grid = named(text, at, grid)
        if case["site"] in ("attr_grid", "attr_grid4"):
            m = re.fullmatch(r"attr_grid\((.+)\)", grid)
            assert m, (kernel, grid)
            per_thread = 1
            if case["site"] == "attr_grid4":
                inner = re.fullmatch(r"ceil_div\(\w+, (\d+)\)", m.group(1))
                assert inner, (kernel, grid)
                per_thread = int(inner.group(1))
                r = re.search(r"void %s\(.*?constexpr int R = (\d+);" % kernel, source("kernels_attr.h"), flags=re.S)
                assert r and int(r.group(1)) == per_thread, (kernel, "destinations per thread")
            else:
                assert re.fullmatch(r"[\w>-]+", m.group(1)), (kernel, grid)
            got.add(attr_grid_cap() * THREADS * per_thread)
        elif case["site"] == "min":
            m = MIN_GRID.match(grid)
            assert m, (kernel, grid)
            got.add(number(m.group(2)) * number(m.group(3)))                  # items per block x the cap
        elif case["site"] == "where":
            body = text[text.index("static void launch_where_ns"):at]
            r = int(re.search(r"constexpr int R = (\d+);", body).group(1))
            m = MIN_GRID.match(re.sub(r"std::max<uint64_t>\(1, (.+)\)$", r"\1", grid))
            assert m and m.group(1) == "nruns", (kernel, grid)
            assert number(m.group(2), {"R": r}) == 4 * r                       # 4 waves of a block, R runs each
            kern = re.search(r"void where_kernel\(.*?\n}\n", source("kernels_attr.h"), flags=re.S).group(0)
            assert "run0 += nwaves * R" in kern and "(run0 + r) * 64 + lane" in kern
            got.add(number(m.group(2), {"R": r}) * 64 * number(m.group(3)))
        else:
            assert case["site"] == "blocks" and grid == "ceil_div(nwords, %d)" % THREADS, (kernel, grid)
            got.add(THREADS * 32)
    assert len(got) == 1, (kernel, got)
    return got.pop()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c["kernels"][0])
def test_the_table_states_what_the_launch_sites_say(case):
    for kernel in case["kernels"]:
        assert per_trip_of(case, kernel) == case["per_trip"], kernel


def test_every_capped_launch_of_these_files_is_in_the_table():
    """A kernel of the four host files launched through attr_grid or a min<uint64_t>(ceil_div(..), CAP) grid is a row of the table, or
    one of those the GPU module's docstring names as out of reach."""
    listed = {k for c in S.CASES for k in c["kernels"]} | set(S.UNCOVERED) | {"batch_side_kernel"}      # (2^20 blocks, as the gathers)
    for name in ("host_attr.h", "host_directory.h", "host_relayout.h", "host_mutate.h"):
        text = source(name)
        for m in re.finditer(r"\b(\w+_kernel)\b(?:<[^<>;()]*>)?<<<", text):
            grid, _, at = [s for s in launches(text, m.group(1)) if s[2] == m.start()][0]
            if re.fullmatch(r"\w+", grid) and not grid.isdigit() and re.search(r"\b%s = " % grid, text[:at]):
                grid = named(text, at, grid)
            if "attr_grid(" in grid or "std::min<uint64_t>" in grid:
                assert m.group(1) in listed, (name, m.group(1), grid)
    m = re.search(r"static uint32_t bitmap_grid\(uint64_t nwords\) \{ return \(uint32_t\)std::min<uint64_t>\(ceil_div\(nwords, (\d+)\), (\d+)\); \}",
                  source("host_relayout.h"))
    assert m and int(m.group(1)) * int(m.group(2)) * 32 == S.UNCOVERED["bitmap_grid"] > 8 * S.N


def test_sizes_are_past_their_thresholds():
    """Every count the GPU module uses: strictly past the first trip, no multiple of 64, and the second trip holds a full run of 64."""
    assert (S.NA, S.NB, S.N, S.N % 64) == (1_100_019, 1_100_018, 2_200_037, 37)
    assert S.N - 2_097_152 == 102_885 and S.N_COMPACT == 2_150_037
    used = 0
    for case in S.CASES:
        for what, sizes in case["sizes"].items():
            for size in sizes:
                assert size > case["per_trip"] and size % 64 != 0 and size - case["per_trip"] >= 64, (case["kernels"], what, size)
                used += 1
    assert used >= 25 and [c["kernels"] for c in S.CASES if not c["sizes"]] == [("bits_differ_kernel",)]
    assert S.K * S.D < 1_048_576                                              # why bits_differ_kernel stays on its first trip
    assert BM.hash_bits(S.NA) == 22 and not BM.is_dense(int(S.HASH_ID(S.NA - 1)) + 1, S.NA) and int(S.HASH_ID(S.NA - 1)) < 2**32
    assert BM.is_dense(S.N, S.N)


# ---- the vectorised models against the per-row ones --------------------------------------------------------------------------------------
def test_columns_are_functions_of_the_id_and_hold_their_edges():
    ids = np.arange(5000, dtype=np.uint64)
    for name, (dtype, edges) in S.COLUMNS.items():
        v = S.column_values(name, ids)
        assert v.dtype == AM.DTYPES[dtype] and np.array_equal(GM.key_image(v[::-1]), GM.key_image(S.column_values(name, ids[::-1])))
        pick = np.array([3000, 17, 4999], dtype=np.uint64)
        assert np.array_equal(GM.key_image(S.column_values(name, pick)), GM.key_image(v[pick.astype(np.int64)]))
        for j, e in enumerate(edges):
            want = GM.key_image(np.array([e]).astype(AM.DTYPES[dtype]) if dtype != "u64" else np.array([e], dtype=np.uint64))[0]
            assert (GM.key_image(v[j::S.EDGE_EVERY]) == want).all(), (name, e)
        assert len(np.unique(GM.key_image(v))) >= 7
    m = S.merged_values(S.B_LACKS, np.array([0, S.NA - 1, S.NA, S.N - 1], dtype=np.uint64))
    assert m[2] == m[3] == S.FILLS[S.B_LACKS] and np.array_equal(m[:2], S.column_values(S.B_LACKS, [0, S.NA - 1]))


def test_where_fast_equals_the_model_and_selects_enough():
    from rabitq_amd import where as W
    ids = np.arange(60_000, dtype=np.uint64)
    cols = {name: (S.COLUMNS[name][0], S.column_values(name, ids)) for name in S.COLUMNS}
    preds = S.predicates()
    assert set(preds) == set(S.NS_OF) and {S.HALF, *S.ANSWERS} <= set(preds)
    assert {S.NS_OF[p] for p in preds} == {(ns, wide) for ns in (1, 2, 4, 8) for wide in (False, True)}
    for name, expr in preds.items():
        terms, prog = W.compile_expr(expr)
        used = {t.column for t in terms}
        ns, wide = S.NS_OF[name]
        assert ns == (1 if len(used) <= 1 else 2 if len(used) <= 2 else 4 if len(used) <= 4 else 8), name      # launch_where's rule
        assert wide == any(S.COLUMNS[c][0] in ("u64", "i64") for c in used), name
        keep = S.where_fast(cols, expr)
        small = {c: (d, v[:3000]) for c, (d, v) in cols.items()}
        slow = AM.where(small, [(t.column, t.op, t.a, t.b, t.values) for t in terms], prog)
        assert np.array_equal(keep[:3000], slow), name
        assert 0.2 < keep.mean() < 0.8, (name, keep.mean())                   # far inside the 1 % .. 99 % the GPU module asserts
    assert 0.45 < S.where_fast(cols, preds[S.HALF]).mean() < 0.55
    terms, prog = W.compile_expr(preds["in4096"])
    assert len(terms[0].values) == 4096
    terms, prog = W.compile_expr(preds["depth32"])
    depth = deepest = 0
    for tok in prog:
        depth += 1 if tok < 32 else (-1 if tok in (AM.TOK_AND, AM.TOK_OR) else 0)
        deepest = max(deepest, depth)
    assert deepest == 32 and AM.program_check(prog, len(terms)) is None
    f = np.array([np.nan, -0.0, 0.0, 2.5, -1.0], dtype=np.float32)            # an f32 set: NaN equals nothing, the zeros are one value
    for members in ([np.nan, 0.0], [-0.0, 2.5], [np.nan], []):
        assert np.array_equal(S.term_fast("f32", f, AM.IN, members=members), AM.term("f32", f, AM.IN, members=members)), members


def test_drop_self_fast_equals_the_model():
    rng = np.random.default_rng(5)
    for topk in (1, 3, 6):
        m, w = 400, topk + 1
        ids = rng.integers(0, 12, size=(m, w)).astype(np.uint32)
        dist = rng.standard_normal((m, w)).astype(np.float32)
        cnt = rng.integers(0, w + 3, size=m).astype(np.uint32)                 # counts past the width are cut to it
        self_ids = rng.integers(0, 12, size=m).astype(np.uint32)
        found = rng.random(m) < 0.8
        for fnd in (None, found):
            a, b = S.drop_self_fast(dist, ids, cnt, self_ids, fnd), BM.drop_self(dist, ids, cnt, self_ids, fnd)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), topk
            assert a[0].dtype == np.float32 and a[1].dtype == np.uint32


def test_set_last_wins_and_keymap_equal_the_models():
    rng = np.random.default_rng(6)
    held = np.arange(0, 600, 2)
    cols = AM.Columns(held)
    cols.create("t", "i64", -4)
    ids = rng.integers(0, 700, size=3000)
    vals = rng.integers(-2**40, 2**40, size=3000)
    absent = cols.set("t", ids, vals)
    uniq, last, gone = S.set_last_wins(ids, vals, np.isin(ids, held))
    assert gone == absent and np.array_equal(uniq, np.unique(ids[np.isin(ids, held)]))
    want, _ = cols.get("t", uniq)
    assert np.array_equal(last, want)
    untouched = held[~np.isin(held, uniq)]
    assert untouched.size and (cols.get("t", untouched)[0] == -4).all()
    map_ids = rng.permutation(5000).astype(np.uint32)
    for name in ("u", "I", "U"):
        fn = lambda i, name=name: S.column_values(name, i)
        whole = GM.keymap_of(map_ids, fn(map_ids))
        ask = rng.choice(map_ids, size=(7, 40))
        part = S.keymap_for(ask, fn)
        assert part == {int(i): whole[int(i)] for i in np.unique(ask)}
