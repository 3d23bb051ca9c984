"""rabitq_amd/csrc/kernel_shapes.h -- the one place that says which instantiations of the width-templated kernels exist -- against
the tables the GPU tests sweep, and the rest of the sources against a second copy of such a list (no GPU: the header is parsed)."""
import glob
import os
import re

from tests import coarse_fused_cases as cf
from tests import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rabitq_amd", "csrc")
NT = {"RQ_NT_W2", "RQ_NT_W12", "RQ_ADD_NT2"}     # the tuning constants of kernels_scan_decl.h a list may name instead of a number


def shape_lists():
    """-> {list name: [tuple of columns]} from the `#define NAME(X) X(..) X(..) ...` lines of the header (numbers as ints)."""
    out = {}
    for name, body in re.findall(r"^#define (RQ_\w+)\(X\) ((?:X\([^)]*\) ?)+)$", open(os.path.join(CSRC, "kernel_shapes.h")).read(), flags=re.M):
        rows = [tuple(int(c) if c.strip().isdigit() else c.strip() for c in row.split(",")) for row in re.findall(r"X\(([^)]*)\)", body)]
        assert all(isinstance(c, int) or c in NT for r in rows for c in r), (name, rows)
        out[name] = rows
    return out


LISTS = shape_lists()
widths = lambda name: [r[0] for r in LISTS[name]]


def test_the_header_holds_the_seven_lists():
    assert set(LISTS) == {"RQ_SCAN_VALU_SHAPES", "RQ_SCAN_MFMA_SHAPES", "RQ_SCAN_MFMA_ADD_SHAPES", "RQ_BF16_TILE_SHAPES",
                          "RQ_COARSE_CAND_SHAPES", "RQ_SMALL_BATCH_WIDTHS", "RQ_RING8_NPC"}
    for name, rows in LISTS.items():
        assert len(rows) == len(set(rows)) and len({len(r) for r in rows}) == 1, (name, rows)
        if name != "RQ_COARSE_CAND_SHAPES":     # (the one family with two shapes of a width)
            assert widths(name) == sorted(set(widths(name))), (name, rows)


def test_scan_widths_are_the_ones_the_scan_tests_sweep():
    assert tuple(widths("RQ_SCAN_VALU_SHAPES")) == sc.WIDTHS
    assert tuple(widths("RQ_SCAN_MFMA_SHAPES")) == sc.WIDTHS
    assert set(widths("RQ_SCAN_MFMA_ADD_SHAPES")) == {1, 2}
    assert set(widths("RQ_SCAN_MFMA_ADD_SHAPES")) <= set(widths("RQ_SCAN_MFMA_SHAPES"))
    assert LISTS["RQ_SCAN_VALU_SHAPES"] == [(1, 2), (2, 2), (3, 2), (4, 2), (6, 2), (8, 2), (12, 1), (16, 1)]
    assert LISTS["RQ_SCAN_MFMA_SHAPES"] == [(1, 4), (2, "RQ_NT_W2"), (3, 4), (4, 2), (6, 2), (8, 2), (12, "RQ_NT_W12"), (16, 2)]
    assert LISTS["RQ_SCAN_MFMA_ADD_SHAPES"] == [(1, 4), (2, "RQ_ADD_NT2")]
    # what tests/test_scan_instantiations_gpu.py is parametrised over: W, on both engines, in both of its tests
    from tests import test_scan_instantiations_gpu as t
    for fn in (t.test_every_instantiation_matches_oracle, t.test_range_search_every_width):
        swept = {m.args[0]: m.args[1] for m in fn.pytestmark if m.name == "parametrize"}
        assert set(swept["W"]) >= set(widths("RQ_SCAN_VALU_SHAPES")) | set(widths("RQ_SCAN_MFMA_SHAPES")), fn.__name__
    assert set(t.ENGINES) == {"valu", "matrix"}


def test_bf16_tile_widths():
    assert LISTS["RQ_BF16_TILE_SHAPES"] == [(1, 2), (2, 2), (3, 1), (4, 1), (6, 1), (8, 1), (12, 1)]


def test_coarse_fused_cases_launch_every_coarse_candidates_shape():
    assert LISTS["RQ_COARSE_CAND_SHAPES"] == [(1, 2), (2, 2), (1, 1), (2, 1), (3, 1), (4, 1)]
    launched = {cf.launched_shape(d, k, LISTS["RQ_COARSE_CAND_SHAPES"]) for d, k, _, _, _ in cf.CASES}
    assert launched == set(LISTS["RQ_COARSE_CAND_SHAPES"]), sorted(launched ^ set(LISTS["RQ_COARSE_CAND_SHAPES"]))
    # two query tiles come before one in the list: the launcher takes the first shape of a width that fits
    for w in set(widths("RQ_COARSE_CAND_SHAPES")):
        nts = [nt for ww, nt in LISTS["RQ_COARSE_CAND_SHAPES"] if ww == w]
        assert nts == sorted(nts, reverse=True) and nts[-1] == 1, (w, nts)


def test_small_batch_and_ring_widths():
    from tests.test_byte_rows_gpu import SB_WIDTHS
    assert tuple(widths("RQ_SMALL_BATCH_WIDTHS")) == SB_WIDTHS == (1, 2, 4, 8, 12, 16)
    assert widths("RQ_RING8_NPC") == [4, 8, 12, 16]     # dim / 16 at dim 64, 128, 192, 256 (tests/test_rerank_ring_gpu.py)


def test_no_other_source_spells_out_a_width_list():
    """Exactly what is looked for, in every Makefile / *.h / *.hip of rabitq_amd/csrc but kernel_shapes.h:
      - a `case 12:` label with a kernel's name (a word ending in `_kernel`, a `launch_*` call, or an `RQ_*(` macro call, which
        is how the launch switches abbreviate a launch) on the same line or the next;
      - the chain `W == 1 || W == 2` (any spacing, and with `idx->W` / `dim` style prefixes of the W).
    12 was a label of every hand-written launch switch and is in no other switch of the sources; every hand-written predicate
    chain began with 1 and 2.  Not covered by this text search: a list without width 12 written out as a switch (the additive
    and coarse_candidates_kernel shapes), and a chain over dimensions (`dim == 64 || dim == 128 ...`, as the ring8 launcher had)."""
    files = [f for pat in ("Makefile", "*.h", "*.hip") for f in glob.glob(os.path.join(CSRC, pat)) if os.path.basename(f) != "kernel_shapes.h"]
    assert len(files) > 25
    found = []
    for f in files:
        lines = open(f).read().split("\n")
        for i, line in enumerate(lines):
            near = line + " " + (lines[i + 1] if i + 1 < len(lines) else "")
            if re.search(r"\bcase\s+12\s*:", line) and re.search(r"\w+_kernel\b|\blaunch_\w+|\bRQ_[A-Z0-9_]+\(", near):
                found.append((os.path.basename(f), i + 1, line.strip()))
            if re.search(r"W\s*==\s*1\s*\|\|\s*[\w>.-]*W\s*==\s*2", line):
                found.append((os.path.basename(f), i + 1, line.strip()))
    assert not found, found


def test_attribute_error_text_names_every_shape():
    """The names ensure_kernel_attributes puts into its error text are generated from the lists; they are what they were when they
    were written out: `kernel<W,NT>` with the NT as a number, but "NT" where the list names a tuning constant.  No test can make
    the attribute call fail, so the strings are looked for in the built library."""
    from rabitq_amd import _lib
    _lib.build()
    blob = open(_lib.SO_PATH, "rb").read()
    nt = lambda v: v if isinstance(v, int) else "NT"
    names = ["scan_mfma_kernel<%d,%s>" % (w, nt(v)) for w, v in LISTS["RQ_SCAN_MFMA_SHAPES"] + LISTS["RQ_SCAN_MFMA_ADD_SHAPES"]]
    names += ["%s<%d,%d>" % (kern, w, v) for kern in ("assign_approx_kernel", "coarse_approx_kernel") for w, v in LISTS["RQ_BF16_TILE_SHAPES"] if w >= 6]
    names += ["coarse_candidates_kernel<%d,%d>" % r for r in LISTS["RQ_COARSE_CAND_SHAPES"]]
    names += ["accurate_ring8_kernel<%d>" % r for r in LISTS["RQ_RING8_NPC"]]
    assert {"scan_mfma_kernel<2,NT>", "scan_mfma_kernel<12,NT>", "scan_mfma_kernel<1,4>", "coarse_approx_kernel<12,1>"} <= set(names)
    missing = [n for n in names if (n + "\0").encode() not in blob]
    assert not missing, missing
    assert not re.search(rb"scan_mfma_kernel<\d+,RQ_", blob) and b"scan_mfma_kernel<2,3>" not in blob and b"scan_mfma_kernel<2,6>" not in blob
