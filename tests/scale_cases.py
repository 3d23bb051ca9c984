"""The bookkeeping kernels whose launch grid is capped (a grid-stride loop takes the rest) or whose blocks are joined on the host, as
data: which kernel, how many items one trip of its grid covers, and the counts tests/test_bookkeeping_scale_gpu.py sends through
it.  tests/test_scale_cases.py parses the launch sites and holds this table to them.  Below the table: the sizes and the column
functions of that module, and the vectorised numpy models it needs at 2.2M rows (pinned to the per-row models by the same CPU test).
Pure numpy: nothing here touches the library or a GPU."""
import numpy as np

from tests import attr_model as AM
from tests import group_model as GM
from tests.by_id_model import ABSENT

# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
D, K = 64, 64
NA, NB = 1_100_019, 1_100_018               # the two halves: each past 1 048 576
N = NA + NB                                 # 2 200 037: past 2 097 152 by 102 885 positions; N % 64 == 37
M_IDS = 2_150_000                           # ids of one by-id request (locate, set_attr, get_attr): past 2 097 152
DEAD = 50_000                               # rows removed lazily, then compacted away
N_COMPACT = N - DEAD                        # 2 150 037: still past 2 097 152
ADDED = 1_000
M_NEIGH = 270_001                           # ids of one neighbours_of call: past 262 144 (the threshold is on m, not n)
N_NEIGH = 3_000                             # rows of the index that call runs on
HASH_ID = lambda i: 7 * np.asarray(i, dtype=np.uint64) + np.uint64(1 << 31)     # ids far apart: the hash directory

# ---- the table ---------------------------------------------------------------------------------------------------------------------------
# kernels: launched the same way at `site`; file: the host file of the launch; site: how the grid is written there --
#   "attr_grid"   <<<attr_grid(count), 256>>>                             one item per thread
#   "attr_grid4"  <<<attr_grid(ceil_div(count, 4)), 256>>>                four items per thread
#   "min"         <<<min<uint64_t>(ceil_div(count, PER_BLOCK), CAP), 256>>>
#   "where"       launch_where_ns: min<uint64_t>(ceil_div(nruns, 4 * R), 2048) blocks of 4 waves, R runs of 64 positions per wave
#   "blocks"      <<<ceil_div(nwords, 256), 256>>>, no cap: 32 positions per word; the boundary between two blocks is what counts
# per_trip: items one trip of the grid (or one block, for "blocks") covers; sizes: {what the count is: the counts the GPU module uses}
CASES = [
    dict(kernels=("filter_block_counts_kernel", "filter_emit_ids_kernel"), file="host_attr.h", site="blocks", per_trip=8_192,
         sizes={"n": (N, N_COMPACT)}),
    dict(kernels=("drop_self_kernel",), file="host_directory.h", site="min", per_trip=262_144, sizes={"m": (M_NEIGH,)}),
    dict(kernels=("attr_fill_kernel",), file="host_attr.h", site="attr_grid", per_trip=524_288, sizes={"n": (NA, NB, N)}),
    dict(kernels=("attr_owner_reset_kernel", "attr_owner_claim_kernel", "attr_scatter_kernel", "attr_fetch_kernel"), file="host_attr.h",
         site="attr_grid", per_trip=524_288, sizes={"m": (NA, NB, M_IDS)}),
    dict(kernels=("filter_id_bits_kernel",), file="host_attr.h", site="attr_grid", per_trip=524_288, sizes={"n": (N,)}),
    dict(kernels=("directory_build_kernel",), file="host_directory.h", site="min", per_trip=1_048_576, sizes={"n": (NA, NB, N, N_COMPACT)}),
    dict(kernels=("id_scan_kernel",), file="host_relayout.h", site="min", per_trip=1_048_576, sizes={"n": (NA, NB, N, N_COMPACT)}),
    dict(kernels=("id_bitmap_kernel",), file="host_mutate.h", site="min", per_trip=1_048_576, sizes={"dst n": (NA, N)}),
    dict(kernels=("id_hits_kernel",), file="host_mutate.h", site="min", per_trip=1_048_576, sizes={"src n": (NB,)}),
    # (count = k * dim or dim * dim words of the two indexes' centroids and rotation: 4096 at the module's shapes -- the second trip
    # needs k * dim > 1 048 576 and stays uncovered)
    dict(kernels=("bits_differ_kernel",), file="host_mutate.h", site="min", per_trip=1_048_576, sizes={}),
    dict(kernels=("directory_lookup_kernel",), file="host_directory.h", site="min", per_trip=2_097_152, sizes={"m": (M_IDS,)}),
    dict(kernels=("where_kernel",), file="host_attr.h", site="where", per_trip=2_097_152, sizes={"n": (N, N_COMPACT)}),
    dict(kernels=("column_gather_kernel",), file="host_attr.h", site="attr_grid4", per_trip=2_097_152,
         sizes={"n_out": (N, N_COMPACT, N_COMPACT + ADDED)}),
]
# what no index of this size reaches (the GPU module's docstring says so): items one trip covers
UNCOVERED = {"bitmap_grid": 4096 * 256 * 32, "fetch_gather_kernel": None, "merge_gather_kernel": None}

# ---- columns: every value a pure function of the id ----------------------------------------------------------------------------------
# name -> (dtype, the edge values): id % EDGE_EVERY == j < len(edges) holds edges[j], every other id a small range (so that every op
# selects something).  Seven columns: one of each type, and two more 4-byte ones for a five-column predicate without a wide column.
EDGE_EVERY = 1009
COLUMNS = {
    "u": ("u32", [0xFFFFFFFF, 0x80000000, 0]),
    "i": ("i32", [-1, -2**31, 2**31 - 1]),
    "f": ("f32", [np.nan, -0.0, 0.0, np.inf, -np.inf]),
    "U": ("u64", [2**64 - 1, 2**63, 2**32, 1]),
    "I": ("i64", [-1, -2**63, 2**63 - 1, 2**32 + 1]),
    "v": ("u32", [0xFFFFFFFF, 0]),
    "w": ("i32", [-2**31, 2**31 - 1]),
}
FILLS = {"u": 0, "i": 0, "f": 0.0, "U": 0, "I": 0, "v": 77, "w": -9}
B_LACKS = "v"                               # the column the second half does not have: its rows hold FILLS["v"] after the merge


def mix(ids, salt):
    """A 64-bit mix of id and salt (splitmix64's finaliser): the pseudo-random part of a column's value."""
    x = np.asarray(ids, dtype=np.uint64) + np.uint64((0x9E3779B97F4A7C15 * (salt + 1)) & (2**64 - 1))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def column_values(name, ids):
    """The value of column `name` for every id of `ids`, in the column's dtype."""
    ids = np.asarray(ids, dtype=np.uint64)
    dtype, edges = COLUMNS[name]
    h = mix(ids, sorted(COLUMNS).index(name))
    if name == "u":
        out = (h % np.uint64(50)).astype(np.uint32)
    elif name == "i":
        out = ((h % np.uint64(40)).astype(np.int64) - 20).astype(np.int32)
    elif name == "f":
        out = (((h % np.uint64(13)).astype(np.int64) - 6) * 0.5).astype(np.float32)
    elif name == "U":
        out = h % np.uint64(53) + np.uint64(2**32 - 3)
    elif name == "I":
        out = (h % np.uint64(2**34)).astype(np.int64) - 2**33
    elif name == "v":
        out = (h % np.uint64(100)).astype(np.uint32)
    else:
        out = ((h % np.uint64(7)).astype(np.int64) - 3).astype(np.int32)
    r = ids % np.uint64(EDGE_EVERY)
    for j, e in enumerate(edges):
        out[r == np.uint64(j)] = np.array([e], dtype=AM.DTYPES[dtype])[0] if dtype != "u64" else np.uint64(e)
    return out


def merged_values(name, ids):
    """Column `name` of the merged index: the rows of the second half hold the fill where that half lacks the column."""
    out = column_values(name, ids)
    if name == B_LACKS:
        out[np.asarray(ids, dtype=np.uint64) >= np.uint64(NA)] = AM.const(COLUMNS[name][0], FILLS[name])
    return out


def predicates():
    """name -> expression: one per instantiation of where_kernel<NS, WIDE> at least -- columns read in {1, 2, 3-4, 5-8} x {no 8-byte
    column, one} --, a set of 4096 members and a program that needs stack depth 32.  Each admits between 1 % and 99 % of the rows."""
    from rabitq_amd import col
    u, i, f, U, I, v, w = (col(c) for c in "uifUIvw")
    deep = u == 31
    for t in range(30, -1, -1):             # u == 0 | (u == 1 | (... | u == 31)): 32 pushes before the first OR
        deep = (u == t) | deep
    return {
        "ns1_narrow": u < 25,
        "ns1_wide": U >= 2**32 + 20,
        "ns2_narrow": (u < 30) & (i < 0),
        "ns2_wide": (u < 40) & (I < 0),
        "ns4_narrow": (u < 40) & (i > -15) & ~(f < -1.0),
        "ns4_wide": ((u < 10) | (i < -10)) | ((f >= 2.0) | (U < 2**32)),
        "ns8_narrow": (u < 40) & (i > -15) & (f < 2.5) & (v != 3) & (w >= -2),
        "ns8_wide": ((u < 40) & (i > -15) & (f < 2.5) & (v != 3) & (w >= -2)) | ((U == 2**64 - 1) | (I == -1)),
        "in4096": i.isin(range(4096)),
        "depth32": deep,
        "f_edges": (f >= 0.0) | ~f.between(-np.inf, np.inf),      # both zeros and +inf; NaN is what no interval holds
    }


NS_OF = {"ns1_narrow": (1, False), "ns1_wide": (1, True), "ns2_narrow": (2, False), "ns2_wide": (2, True), "ns4_narrow": (4, False),
         "ns4_wide": (4, True), "ns8_narrow": (8, False), "ns8_wide": (8, True), "in4096": (1, False), "depth32": (1, False),
         "f_edges": (1, False)}
HALF = "ns1_narrow"                          # admits about half the rows (u < 25 of 0 .. 49)
ANSWERS = ("ns4_wide", "ns8_narrow", "in4096")   # the predicates whose query answers are compared with the id-list filter's


# ---- vectorised models -----------------------------------------------------------------------------------------------------------------
def term_fast(dtype, values, op, a=0, b=0, members=()):
    """attr_model.term, with the set of an IN term looked up at once (an f32 set: -0 == +0 and NaN equals nothing, as == has it)."""
    if op != AM.IN:
        return AM.term(dtype, values, op, a, b, members)
    v = np.asarray(values, dtype=AM.DTYPES[dtype])
    s = np.array([AM.const(dtype, m) for m in members], dtype=AM.DTYPES[dtype])
    if dtype == "f32":
        s = s[s == s] + np.float32(0.0)
        return np.isin(v + np.float32(0.0), s) & (v == v)
    return np.isin(v, s)


def where_fast(columns, expr):
    """columns {name: (dtype, values)} and an expression of rabitq_amd.where -> the admitted rows (bool)."""
    from rabitq_amd import where as W
    terms, prog = W.compile_expr(expr)
    n = len(next(iter(columns.values()))[1])
    truths = [term_fast(columns[t.column][0], columns[t.column][1], t.op, t.a, t.b, t.values) for t in terms]
    return AM.evaluate(prog, truths, n)


def drop_self_fast(dist, ids, cnt, self_ids, found=None):
    """by_id_model.drop_self for every row at once."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.uint32)
    m, w = ids.shape
    topk = w - 1
    n = np.minimum(np.asarray(cnt, dtype=np.int64), w)
    if found is not None:
        n = np.where(np.asarray(found, dtype=bool), n, 0)
    e = np.arange(w)[None, :]
    hit = (ids == np.asarray(self_ids, dtype=np.uint32)[:, None]) & (e < n[:, None])
    drop = np.where(hit.any(1), hit.argmax(1), n - 1)                         # (n == 0: -1, and nothing is valid)
    src = np.arange(topk)[None, :]
    src = np.where(src < drop[:, None], src, src + 1)
    valid = src < n[:, None]
    at = np.minimum(src, w - 1)
    od = np.where(valid, np.take_along_axis(dist.view(np.uint32), at, 1), np.uint32(0)).astype(np.uint32).view(np.float32)
    od[~valid] = np.nan
    oi = np.where(valid, np.take_along_axis(ids, at, 1), np.uint32(ABSENT)).astype(np.uint32)
    return od, oi


def set_last_wins(ids, values, present):
    """rq_attr_set's rule: -> (unique present ids, the value each ends with: its last occurrence's, absent requests).  present: a
    boolean per request -- the index holds a live row of that id."""
    ids, values, present = np.asarray(ids), np.asarray(values), np.asarray(present, dtype=bool)
    absent = int((~present).sum())
    ids, values = ids[present], values[present]
    uniq, first_of_reversed = np.unique(ids[::-1], return_index=True)
    return uniq, values[::-1][first_of_reversed], absent


def keymap_for(ids, values_of):
    """{id: key image} for the ids of a source call's rows alone (values_of: ids -> the column's values)."""
    uniq = np.unique(np.asarray(ids, dtype=np.uint32))
    return dict(zip(uniq.tolist(), GM.key_image(values_of(uniq)).tolist()))
