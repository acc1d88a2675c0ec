"""A device-free model of one index handle, a generator of mutation sequences for it, the table of search calls that read the
handle's derived state, and the comparison of one call's results on two handles.

The contract under test ("derived state"): an answer depends only on the stored rows, the labels, the options and
the call's arguments -- not on how the index got there, nor on which derived copies existed when it was changed.  So a handle
that went through any history answers bit for bit like one built from the final rows in one ``add``.

``Model`` restates the eight mutations in plain numpy.  ``ops(seed, metric, d)`` returns a replayable list of plain tuples;
``trace`` replays a list through the model and names, per op, the state of the copies it met and the special forms it is.
``call_table`` lists the search calls of a checkpoint; ``compare`` checks one call's results on two handles;
``reference_check`` holds a result against float64 scores of the model's rows.  numpy and ``wdbx_oracle`` only.
"""
import numpy as np

import wdbx_oracle as O

LABEL_NONE = 0xFFFFFFFF
K, NQ = 2, 16
INITIAL_CAPACITY = 1024          # of the mutated handle: below every first add, so the first add already grows it
N_MIN, N_MAX = 2100, 4000        # the row count at every checkpoint: k * 8 * 128 = 2 048 rows keep every selection route eligible
ADD_SIZES = (1, 63, 64, 65, 300)
KINDS = ("add", "reserve", "set_rows", "set_rows_at", "remove_rows", "set_labels", "compact", "clear")
STATES = ("never built", "lagging", "warm")

# the option sets of tests/test_gpu_update.py (test_index_model_host.py holds them equal)
BASE = {"single_min_rows": 0, "gemm_min_rows": 0, "gemm_min_work": 1, "gemm_min_queries": 4, "scan_shadow": 2, "scan_u6": 0,
        "scan_u42": 0, "gemm_bf16": 3}
ROUTES = [
    ("u8 scan", {"gemm_min_queries": 1 << 30}, 1),
    ("u6 rounds", {"gemm_min_queries": 1 << 30, "scan_u6": 1}, NQ),
    ("u42 rounds", {"gemm_min_queries": 1 << 30, "scan_u6": 1, "scan_u42": 1}, NQ),
    ("i8 tiles", {"gemm_bf16": 3}, NQ),
    ("bf16 shadow tiles", {"gemm_bf16": 2}, NQ),
    ("bf16 tiles", {"gemm_bf16": 1}, NQ),
    ("fp32 tiles", {"gemm_bf16": 0}, NQ),
    ("fp32 scan", {"gemm_min_queries": 1 << 30, "scan_shadow": 0}, 1),
]
# what the library reports after a route ran: {option: value}.  On a fresh handle, whose reports start at zero, each differs
# from what the routes before it in ROUTES leave behind, so reading it back there shows that the route ran.
ROUTE_REPORTS = {
    "u8 scan": {"last_single_path": 2, "last_single_u6": 0},
    "u6 rounds": {"last_single_path": 2, "last_single_u6": 1, "last_single_u42": 0},
    "u42 rounds": {"last_single_path": 2, "last_single_u6": 1, "last_single_u42": 1},
    "i8 tiles": {"last_gemm_family": 3},
    "bf16 shadow tiles": {"last_gemm_family": 2},
    "bf16 tiles": {"last_gemm_family": 1},
    "fp32 tiles": {"last_gemm_family": 0},
    "fp32 scan": {"last_single_path": 0},
}
COSINE_ONLY = ("u6 rounds", "u42 rounds")   # u6_single_eligible refuses L2: their option sets run the u8 rounds there


def route_report(name, metric):
    """what the library reports after the route's option set ran on an index of this metric"""
    if metric == "l2" and name in COSINE_ONLY:
        return {key: 2 if key == "last_single_path" else 0 for key in ROUTE_REPORTS[name]}
    return ROUTE_REPORTS[name]


def routes_of(metric):
    return {name for name, _, _ in ROUTES if metric == "cosine" or name not in COSINE_ONLY}


COVERAGES = ("shadow_rows", "shadowg_rows", "shadow8_rows", "shadow6_rows", "shadow42_rows")

# the committed sequences: (seed, d) per metric, d = 384 for one of them (test_index_model_host.py asserts what they cover)
SEEDS = {
    "cosine": [(1, 96), (6, 96), (17, 96), (30, 96), (32, 96), (0, 384)],
    "l2": [(0, 96), (1, 96), (3, 96), (7, 96), (12, 96), (0, 384)],
}


def queries_for(d, metric):
    q = O.synth_rows(O.SEED_QUERY, 0, NQ, d).astype(np.float32)
    return O.normalize_rows_fast(q) if metric == "cosine" else q


def data(dseed, n, d, metric, scale=1.0):
    """the n rows an op with data seed dseed writes"""
    rows = np.random.default_rng(dseed).standard_normal((n, d)).astype(np.float32)
    if metric == "cosine":
        return O.normalize_rows_fast(rows)
    return (rows * np.float32(scale)).astype(np.float32)


def labels_for(lseed, n):
    """n labels out of 40, one in ten 'a label of its own'"""
    rng = np.random.default_rng(lseed)
    lab = rng.integers(0, 40, n).astype(np.uint32)
    lab[rng.random(n) < 0.1] = LABEL_NONE
    return lab


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model:
    """rows float32 [n, d]; labels uint32 [n], or None while no label was ever set (since creation or the last clear)"""

    def __init__(self, d, metric, capacity=INITIAL_CAPACITY):
        self.d, self.metric = d, metric
        self.rows = np.empty((0, d), np.float32)
        self.labels = None
        self.cap = capacity
        self.queries = queries_for(d, metric)

    @property
    def n(self):
        return len(self.rows)

    # the eight mutations
    def add(self, rows):
        if self.n + len(rows) > self.cap:        # (how the handle grows: the need, or half as much again)
            self.cap = max(self.n + len(rows), self.cap + self.cap // 2)
        self.rows = np.concatenate([self.rows, rows])
        if self.labels is not None:              # rows added since the last set_labels are labels of their own
            self.labels = np.concatenate([self.labels, np.full(len(rows), LABEL_NONE, np.uint32)])

    def reserve(self, capacity):
        self.cap = max(self.cap, capacity)

    def set_rows(self, first, rows):
        self.rows[first:first + len(rows)] = rows

    def set_rows_at(self, ids, rows):
        self.rows[np.asarray(ids, np.int64)] = rows

    def remove_rows(self, ids):
        self.rows[np.asarray(ids, np.int64)] = np.nan

    def set_labels(self, first, labels):
        if self.labels is None:
            self.labels = np.full(self.n, LABEL_NONE, np.uint32)
        self.labels[first:first + len(labels)] = labels

    def compact(self, keep):
        keep = np.asarray(keep, np.int64)
        self.rows = self.rows[keep]
        if self.labels is not None:
            self.labels = self.labels[keep]

    def clear(self):
        self.rows = np.empty((0, self.d), np.float32)
        self.labels = None

    # an op of ops(): its concrete arguments (arrays), for the model and for a handle alike
    def concrete(self, op):
        kind = op[0]
        if kind == "add":
            return kind, (data(op[2], op[1], self.d, self.metric),)
        if kind == "reserve":
            return kind, (op[1],)
        if kind == "set_rows":
            return kind, (op[1], data(op[3], op[2], self.d, self.metric, op[4]))
        if kind == "set_rows_at":
            _, ids, dseed, nan_pos, zero_pos, planted, _ = op
            rows = data(dseed, len(ids), self.d, self.metric)
            if nan_pos >= 0:
                rows[nan_pos] = np.nan
            if zero_pos >= 0:
                rows[zero_pos] = 0.0
            for pos, qi in planted:
                rows[pos] = self.queries[qi]
            return kind, (np.asarray(ids, np.uint64), rows)
        if kind == "remove_rows":
            return kind, (np.asarray(op[1], np.uint64),)
        if kind == "set_labels":
            return kind, (op[1], labels_for(op[3], op[2]))
        if kind == "compact":
            return kind, (self.keep_of(op),)
        if kind == "clear":
            return kind, ()
        raise ValueError(op)

    def keep_of(self, op):
        _, form, a, b, _ = op
        if form == "prefix":                     # nothing moves, the live tail rows are dropped
            return np.arange(a, dtype=np.uint64)
        if form == "scattered":
            drop = np.random.default_rng(a).choice(self.n, b, replace=False)
            return np.setdiff1d(np.arange(self.n, dtype=np.uint64), drop.astype(np.uint64))
        if form == "tombstones":                 # exactly the removed rows go
            return np.flatnonzero(~self.removed()).astype(np.uint64)
        raise ValueError(op)

    def apply(self, op):
        kind, args = self.concrete(op)
        getattr(self, kind)(*args)
        return kind, args

    def removed(self):
        """bool [n]: rows that are never a result (a NaN element)"""
        return np.isnan(self.rows).any(axis=1)

    def planted(self):
        """{query: row}: the smallest row that is a bit-for-bit copy of query 0 .. 3 (it wins that query on every route:
        equal scores rank by row)"""
        out = {}
        for qi in range(4):
            same = np.flatnonzero((self.rows.view(np.uint32) == self.queries[qi].view(np.uint32)).all(axis=1))
            if len(same):
                out[qi] = int(same[0])
        return out


def apply_to_handle(ix, kind, args):
    """the same concrete op on a NativeIndex"""
    getattr(ix, kind)(*args)


# ---- bookkeeping of the copies' state along a sequence ------------------------------------------------------------------
class Trace:
    """Replays ops through a Model and notes, per op, the state of the copies when it ran and the special forms it is.
    built: the routes were searched at least once since creation; cov: the row count the copies cover at the most (the row
    count at the last warm point, cut by compact to its first moved row and by clear to 0)."""

    def __init__(self, d, metric):
        self.m = Model(d, metric)
        self.built, self.cov, self.prev_warm = False, 0, False
        self.prev = None
        self.labels_appended = False   # rows were added since labels were last set
        self.cleared_from = None       # the row count a clear dropped, until the next add
        self.outlier = None            # bits of the outlier row while it is stored
        self.log = []                  # (kind, state, forms)

    def state(self):
        if not self.built:
            return "never built"
        return "warm" if self.prev_warm else "lagging"

    def step(self, op):
        m, kind, warm = self.m, op[0], bool(op[-1])
        state, forms, n = self.state(), set(), self.m.n
        edge = self.built and 0 < self.cov < n
        if kind == "add":
            forms.add("add %d" % op[1] if op[1] in ADD_SIZES else "add many")
            if n + op[1] > m.cap:
                forms.add("add beyond the capacity")
            if self.prev is not None and self.prev[0] == "add" and not self.prev[-1]:
                forms.add("add after add, no search between")
            if m.labels is not None:
                forms.add("rows appended after set_labels")
                self.labels_appended = True
            if self.cleared_from is not None:
                if op[1] < self.cleared_from and op[1] % 256:
                    forms.add("clear, then fewer rows")
                self.cleared_from = None
        elif kind == "reserve":
            forms.add("reserve beyond the capacity" if op[1] > m.cap else "reserve")
        elif kind == "set_rows":
            first, count = op[1], op[2]
            if first // 64 != (first + count - 1) // 64:
                forms.add("set_rows across a group boundary")
            if edge and first < self.cov < first + count:
                forms.add("set_rows across a coverage edge")
            if edge and first >= self.cov:
                forms.add("set_rows behind every coverage")
            if op[4] != 1.0:
                forms.add("outlier norm")
            elif self.outlier is not None and count == 1 and np.array_equal(m.rows[first].view(np.uint32), self.outlier):
                forms.add("outlier overwritten back")
        elif kind in ("set_rows_at", "remove_rows"):
            ids = np.asarray(op[1])
            if ids[0] == 0 and ids[-1] == n - 1 and np.any(ids % 64 == 63) and np.any((ids % 64 == 0) & (ids > 0)):
                forms.add(kind + " list with rows 0, 63 and 0 mod 64, last")
            if edge and np.any((ids >= self.cov - 64) & (ids < self.cov)) and np.any((ids >= self.cov) & (ids < self.cov + 64)):
                forms.add(kind + " list on both sides of a coverage edge")
            if kind == "set_rows_at":
                if op[3] >= 0:
                    forms.add("list with a NaN row")
                if op[4] >= 0:
                    forms.add("list with a zero row")
                if sorted(qi for _, qi in op[5]) == [0, 1, 2, 3]:
                    forms.add("list with planted rows")
        elif kind == "set_labels":
            if m.labels is None:
                forms.add("first set_labels")
            elif self.labels_appended:
                forms.add("relabel after rows were appended")
            self.labels_appended = False
        elif kind == "compact":
            keep = m.keep_of(op)
            moved = np.flatnonzero(keep != np.arange(len(keep)))
            first_moved = int(moved[0]) if len(moved) else len(keep)
            if op[1] == "prefix" and len(keep) < n and not m.removed()[len(keep):].all():
                forms.add("compact to a prefix")
            if op[1] == "scattered" and len(moved):
                forms.add("compact scattered")
            if op[1] == "tombstones" and len(keep) < n:
                forms.add("compact exactly the tombstones")
        elif kind == "clear":
            self.cleared_from = n
        # the model, then the copies' reach
        _, args = m.apply(op)
        if kind == "set_rows" and op[4] != 1.0:
            self.outlier = m.rows[op[1]].view(np.uint32).copy()
        elif kind != "reserve" and self.outlier is not None and not (m.rows.view(np.uint32) == self.outlier).all(axis=1).any():
            self.outlier = None
        if kind == "compact":
            self.cov = min(self.cov, first_moved)
        if kind == "clear":
            self.cov = 0
            self.labels_appended = False
        if warm and m.n:
            self.built, self.cov = True, m.n
        self.prev_warm = warm and m.n > 0
        self.prev = op
        self.log.append((kind, state, frozenset(forms)))
        return state, forms


def trace(seq, metric, d):
    t = Trace(d, metric)
    for op in seq:
        t.step(op)
    return t.log


def cells(seqs):
    """seqs: [(seq, metric, d)].  Returns ({(mutation kind, state of the copies)}, {special form}) that occurred."""
    hit, forms = set(), set()
    for seq, metric, d in seqs:
        for kind, state, f in trace(seq, metric, d):
            hit.add((kind, state))
            forms |= f
    return hit, forms


FORMS = (
    ["add %d" % s for s in ADD_SIZES] + [
        "add beyond the capacity", "add after add, no search between", "reserve beyond the capacity",
        "set_rows across a group boundary", "set_rows across a coverage edge", "set_rows behind every coverage",
        "set_rows_at list with rows 0, 63 and 0 mod 64, last", "remove_rows list with rows 0, 63 and 0 mod 64, last",
        "set_rows_at list on both sides of a coverage edge", "remove_rows list on both sides of a coverage edge",
        "list with a NaN row", "list with a zero row", "list with planted rows",
        "first set_labels", "rows appended after set_labels", "relabel after rows were appended",
        "compact to a prefix", "compact scattered", "compact exactly the tombstones", "clear, then fewer rows"])
FORMS_L2 = ["outlier norm", "outlier overwritten back"]


# ---- the generator ------------------------------------------------------------------------------------------------------
def ops(seed, metric, d):
    """10 .. 14 ops: plain tuples, the last element the flag ``warm`` (every route is searched before the next mutation).
      ("add", rows, data seed, warm)                      ("reserve", capacity, warm)
      ("set_rows", first, rows, data seed, scale, warm)   ("remove_rows", ids, warm)
      ("set_rows_at", ids, data seed, position of the NaN row, of the zero row, ((position, query) planted), warm)
      ("set_labels", first, rows, label seed, warm)       ("clear", False)
      ("compact", "prefix" | "scattered" | "tombstones", rows kept | seed | 0, rows dropped | 0, warm)
    The same arguments always give the same list."""
    rng = np.random.default_rng([seed, 0 if metric == "cosine" else 1, d])
    t = Trace(d, metric)
    m = t.m
    seq = []

    def emit(*op):
        op = tuple(op)
        seq.append(op)
        t.step(op)
        assert op[0] == "clear" or N_MIN <= m.n <= N_MAX, (seed, metric, d, seq)

    def dseed():
        return int(rng.integers(1, 1 << 30))

    def edge():
        return t.built and 0 < t.cov < m.n

    def add(count, warm):
        emit("add", int(count), dseed(), warm)

    def set_rows(warm):
        n = m.n
        forms = ["group"]
        if edge():
            forms += ["straddle", "behind", "straddle", "behind"]
        form = forms[int(rng.integers(len(forms)))]
        if form == "straddle":
            first = max(0, t.cov - int(rng.integers(1, 40)))
            count = min(n - first, t.cov - first + int(rng.integers(1, 40)))
        elif form == "behind":
            first = int(rng.integers(t.cov, n))
            count = int(rng.integers(1, n - first + 1))
        else:
            first = 64 * int(rng.integers(1, n // 64)) - int(rng.integers(1, 20))
            count = min(n - first, int(rng.integers(21, 90)))
        emit("set_rows", first, count, dseed(), 1.0, warm)

    def row_list():
        n = m.n
        ids = {0, n - 1, 64 * int(rng.integers(0, (n - 64) // 64)) + 63, 64 * int(rng.integers(1, n // 64))}
        special = sorted(ids)
        if edge():
            g = t.cov // 64 * 64
            ids |= {t.cov - 1, t.cov, min(n - 1, t.cov + 1)} | ({g - 1, g} if g > 0 else set())
        ids |= set(int(r) for r in rng.choice(n, 30, replace=False))
        return tuple(sorted(ids)), special

    def set_rows_at(warm):
        ids, special = row_list()
        free = [i for i, r in enumerate(ids) if r not in special]
        nan_pos, zero_pos = (int(p) for p in rng.choice(free, 2, replace=False))
        planted = tuple((ids.index(r), qi) for qi, r in enumerate(special))
        emit("set_rows_at", ids, dseed(), nan_pos, zero_pos, planted, warm)

    def remove_rows(warm):
        emit("remove_rows", row_list()[0], warm)

    def set_labels(warm):
        n = m.n
        first = int(rng.integers(0, n // 2))
        count = int(rng.integers(n // 4, n - first + 1))
        emit("set_labels", first, count, dseed(), warm)

    def compact(warm, form=None):
        n = m.n
        room = n - N_MIN
        gone = int(m.removed().sum())
        forms = [f for f in ("prefix", "scattered") if room >= 10] + (["tombstones"] * 2 if 0 < gone <= room else [])
        if not forms:
            return add(300, warm)
        form = form if form in forms else forms[int(rng.integers(len(forms)))]
        if form == "prefix":
            emit("compact", "prefix", n - int(rng.integers(5, min(150, room) + 1)), 0, warm)
        elif form == "scattered":
            emit("compact", "scattered", dseed(), int(rng.integers(5, min(150, room) + 1)), warm)
        else:
            emit("compact", "tombstones", 0, 0, warm)

    def clear_add(warm):
        n = m.n
        if n < N_MIN + 20:
            return add(300, warm)
        fewer = n - int(rng.integers(10, min(400, n - N_MIN)))
        fewer -= 1 if fewer % 256 == 0 else 0
        emit("clear", False)
        add(fewer, warm)

    def reserve(warm):
        emit("reserve", m.cap + int(rng.integers(1, 700)), warm)

    def outlier(warm):
        emit("set_rows", int(rng.integers(1, m.n)), 1, dseed(), 100.0, warm)

    def outlier_back(warm):
        if t.outlier is None:
            return set_rows(warm)
        row = int(np.flatnonzero((m.rows.view(np.uint32) == t.outlier).all(axis=1))[0])
        emit("set_rows", row, 1, dseed(), 1.0, warm)

    def flag():
        return bool(rng.random() < 0.5)

    # before the first search: the first add (beyond the capacity), then two more mutations that meet no copy at all
    add(rng.integers(2300, 2700), False)
    never = [(lambda w: add(63, w), set_rows), (set_rows_at, remove_rows), (set_labels, lambda w: compact(w, "scattered")),
             (reserve, clear_add), (lambda w: add(1, w), set_rows_at), (lambda w: compact(w, "prefix"), set_labels),
             (remove_rows, lambda w: compact(w, "tombstones"))][int(rng.integers(7))]
    never[0](False)
    never[1](True)
    # then every kind, each met by warm or by lagging copies as the flags fall
    sizes = [int(s) for s in rng.permutation(ADD_SIZES)]
    body = [lambda w: (add(sizes[0], False), add(sizes[1], w)), set_rows_at, remove_rows, compact, set_rows, set_labels]
    extras = [reserve, clear_add, set_labels, set_rows, lambda w: add(sizes[2], w), compact, remove_rows]
    body += [extras[int(i)] for i in rng.choice(len(extras), 2, replace=False)]
    order = [int(i) for i in rng.permutation(len(body))]
    body = [body[i] for i in order]
    if metric == "l2":                         # the outlier and, two or more items later, its overwrite
        at = int(rng.integers(0, len(body) - 2))
        body.insert(at, outlier)
        body.insert(int(rng.integers(at + 2, len(body) + 1)), outlier_back)
    for item in body:
        if len(seq) >= 13:
            break
        item(flag())
    assert 10 <= len(seq) <= 14, (seed, metric, d, len(seq))
    return seq


# ---- the call table -----------------------------------------------------------------------------------------------------
def range_threshold(d, metric):
    """a threshold some 2 % of standard-normal rows reach: two standard deviations of the score from its mean"""
    if metric == "cosine":
        return np.float32(2.0 / np.sqrt(d))
    return np.float32(2.0 * d - 2.0 * np.sqrt(6.0 * d))


def pack_row_mask(allowed):
    padded = np.zeros((len(allowed) + 31) // 32 * 32, dtype=bool)
    padded[:len(allowed)] = allowed
    return np.packbits(padded, bitorder="little").view(np.uint32)


def listed_rows(model, recent, rng, count=40):
    """count row numbers, strictly increasing: the recently written, removed and appended rows first, random ones beside"""
    n = model.n
    take = sorted(set(int(r) for r in recent if r < n))[:count // 2]
    rest = np.setdiff1d(np.arange(n), take)
    ids = np.concatenate([np.asarray(take, np.int64), rng.choice(rest, count - len(take), replace=False)])
    return np.sort(ids).astype(np.uint64)


def recent_rows(model, kind, args):
    """the rows the op (already applied) wrote, removed or appended -- what search_rows lists at the next checkpoint"""
    n = model.n
    if kind == "add":
        return list(range(max(0, n - len(args[0])), n))[-12:]
    if kind == "set_rows":
        return list(range(args[0], args[0] + len(args[1])))[:12]
    if kind in ("set_rows_at", "remove_rows"):
        return [int(r) for r in args[0]][:20]
    return []


def call_table(model, recent, full=True):
    """[(name, options over BASE, fn(ix) -> tuple of arrays, kind, options the library reports the call's path in, what
    reference_check takes for it or None)].
    kind: "topk" (row ids first, scores second), "range" (offsets, rows, scores) or "other" (row ids first).  Every argument
    is fixed by the model's row count and a seed of it, so two handles get the same calls.  full=False: the eight routes only."""
    n, d, q = model.n, model.d, model.queries
    rng = np.random.default_rng(n)
    route_opts = {name: opts for name, opts, _ in ROUTES}
    per_call = {name: per for name, _, per in ROUTES}

    def chunks(name, fn):
        """fn over the queries, per_call of the route at a time"""
        def run(ix):
            got = [fn(ix, q[q0:q0 + per_call[name]]) for q0 in range(0, NQ, per_call[name])]
            return tuple(np.concatenate([g[i] for g in got]) for i in range(len(got[0])))
        return run

    table = [("search, " + name, opts, chunks(name, lambda ix, qq: ix.search(qq, K)), "topk", tuple(ROUTE_REPORTS[name]))
             for name, opts, _ in ROUTES]
    if not full:
        return _with_references(table)
    mask = pack_row_mask(rng.random(n) < 0.5)
    masks = [pack_row_mask(rng.random(n) < f) for f in (0.5, 0.1, 0.9)]
    which = np.arange(NQ, dtype=np.int32) % 4 - 1
    ids = listed_rows(model, recent, rng)
    lists = [ids, ids[::6], np.empty(0, np.uint64)]
    thr = range_threshold(d, model.metric)
    table += [
        ("search k=200, fp32 scan", route_opts["fp32 scan"],
         lambda ix: tuple(np.concatenate(x) for x in zip(*[ix.search(q[i:i + 1], 200) for i in range(2)])), "topk", ("last_single_path",)),
        ("masked search, u8 scan", route_opts["u8 scan"],
         lambda ix: tuple(np.concatenate(x) for x in zip(*[ix.search(q[i:i + 1], K, mask_words=mask) for i in range(2)])), "topk",
         ("last_single_path",)),
        ("masked search, i8 tiles", route_opts["i8 tiles"], lambda ix: ix.search(q, K, mask_words=mask), "topk",
         ("last_batch_masked", "last_gemm_family")),
        ("search_multimask", route_opts["i8 tiles"], lambda ix: ix.search_multimask(q, K, masks, which), "topk",
         ("last_batch_masked", "last_batch_mask_classes")),
        ("search_rows", {}, lambda ix: ix.search_rows(q, 5, ids), "topk", ("last_rows_path",)),
        ("search_row_lists", {}, lambda ix: ix.search_row_lists(q, 5, lists, np.arange(NQ, dtype=np.int32) % 3), "topk",
         ("last_lists_path", "last_lists_items", "last_lists_rounds")),
        ("search_matrix", {}, lambda ix: ix.search_matrix(ids, 3), "topk", ("last_matrix_path", "last_matrix_rounds")),
        ("search_mmr", {}, lambda ix: ix.search_mmr(q[:4], 5, 20, 0.5), "topk", ("last_mmr_path", "last_mmr_rounds", "last_mmr_candidates")),
        ("search_recommend", {}, lambda ix: ix.search_recommend(q[:12], [0, 2, 3, 5, 6, 9, 12], 5, exclude_rows=ids[:3]), "topk",
         ("last_recommend_path", "last_recommend_short")),
        ("search_discover", {}, lambda ix: ix.search_discover(q[:2], q[2:10], [0, 2, 4], 5), "topk", ("last_discover_path",)),
        ("search_discover, context only", {}, lambda ix: ix.search_discover(None, q[2:10], [0, 2, 4], 5), "topk", ("last_discover_path",)),
        ("range_search", {}, lambda ix: ix.range_search(q[:4], thr), "range", ("last_range_path",)),
        ("range_search_batch", route_opts["i8 tiles"], lambda ix: ix.range_search_batch(q, thr), "range",
         ("last_range_batch_path", "last_range_batch_blocks", "last_range_batch_fallback_queries")),
    ]
    if model.labels is not None:
        slot_labels = ((np.arange(NQ)[:, None] + np.arange(3)[None, :]) % 40).astype(np.uint32)
        slot_labels[:, 2] = LABEL_NONE                       # the single row slot_rows
        slot_rows = np.tile(np.array([0, -1, int(ids[1])], np.int64), (NQ, 1))    # (the middle slot is unused)
        table += [
            ("search_distinct", {}, lambda ix: ix.search_distinct(q, 5), "topk",
             ("last_distinct_path", "last_distinct_items", "last_distinct_labels", "last_distinct_short")),
            ("search_distinct, masked", {}, lambda ix: ix.search_distinct(q[:3], 5, mask_words=mask), "topk", ("last_distinct_path",)),
            ("search_groups", {}, lambda ix: ix.search_groups(q[:8], 3, 4), "topk", ("last_groups_path", "last_groups_tasks", "last_groups_rounds")),
            ("search_group_members", {}, lambda ix: ix.search_group_members(q, slot_labels, slot_rows, 4), "topk", ("last_groups_path",)),
            ("search_multivector", {}, lambda ix: ix.search_multivector(q, [0, 3, 8, 16], 4), "topk",
             ("last_multivector_rounds", "last_multivector_vectors", "last_multivector_labels")),
        ]
    return _with_references(table, ids, thr)


def _with_references(table, ids=None, thr=None):
    """each entry with a sixth field: None, or (name, arguments) for reference_check"""
    refs = {"search_rows": ("search_rows", {"listed": ids}), "range_search": ("range_search", {"thresholds": thr}),
            "search_distinct": ("search_distinct", {})}
    return [e + (("search", {}) if e[0].startswith("search, ") else refs.get(e[0]),) for e in table]


def run_call(ix, entry):
    """one entry of call_table on a handle: (its results, what the library reports about its path)"""
    _, opts, fn, _, reports, _ = entry
    for key, value in {**BASE, **opts}.items():
        ix.set_option(key, value)
    got = fn(ix)
    return tuple(np.asarray(a) for a in got), {r: ix.get_option(r) for r in reports}


# ---- the checker --------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _by_id(got):
    """a range result with every query's rows in row order"""
    offsets, rows, scores = got
    rows, scores = rows.copy(), scores.copy()
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        order = np.argsort(rows[a:b], kind="stable")
        rows[a:b], scores[a:b] = rows[a:b][order], scores[a:b][order]
    return offsets, rows, scores


def compare(got_a, got_f, call="", kind="topk", ordered=True):
    """None when the two results of one call are equal in ids and in score bits, else a description of the first difference:
    the call (its route is part of the name), the query, the position, both values.  Range results whose order the header
    does not promise (ordered=False) are put in row order first."""
    if kind == "range":
        if not ordered:
            got_a, got_f = _by_id(got_a), _by_id(got_f)
        off_a, off_f = got_a[0], got_f[0]
        for qi in range(len(off_a) - 1):
            for what, a, f in (("row", got_a[1], got_f[1]), ("score bits", _bits(got_a[2]), _bits(got_f[2]))):
                ra, rf = a[int(off_a[qi]):int(off_a[qi + 1])], f[int(off_f[qi]):int(off_f[qi + 1])]
                m = min(len(ra), len(rf))
                diff = np.flatnonzero(ra[:m] != rf[:m])
                if len(diff):
                    p = int(diff[0])
                    return f"{call}: query {qi}, position {p}: {what} {ra[p]} on the mutated handle, {rf[p]} on the fresh one"
                if len(ra) != len(rf):
                    return (f"{call}: query {qi}, position {m}: {len(ra)} rows on the mutated handle, {len(rf)} on the fresh one "
                            f"(first extra {what}: {(ra if len(ra) > m else rf)[m]})")
        return None
    if len(got_a) != len(got_f):
        return f"{call}: {len(got_a)} result arrays on the mutated handle, {len(got_f)} on the fresh one"
    for part, (a, f) in enumerate(zip(got_a, got_f)):
        if a.shape != f.shape:
            return f"{call}: result {part} has shape {a.shape} on the mutated handle, {f.shape} on the fresh one"
        a, f = _bits(a), _bits(f)
        diff = np.argwhere(a != f)
        if len(diff):
            at = tuple(int(x) for x in diff[0])
            what = "row" if part == 0 else "score bits" if part == 1 else f"result {part}"
            return (f"{call}: query {at[0]}, position {at[1:] if len(at) != 2 else at[1]}: {what} {a[at]} on the mutated handle, "
                    f"{f[at]} on the fresh one")
    return None


# ---- the float64 reference ----------------------------------------------------------------------------------------------
def gamma(pitch):
    """the library's own coefficient of an fp32 chain of pitch + 18 terms (``nu`` in the batched path of host_index.h)"""
    mu = (pitch + 18) * 2.0 ** -24
    return mu / (1.0 - mu)


def scores64(rows, query, metric):
    """(score to rank by, descending; S: what the fp32 error of the score is relative to) per row, in float64; removed rows
    score -inf with S = 0"""
    r, q = rows.astype(np.float64), query.astype(np.float64)
    if metric == "cosine":
        s, big = r @ q, np.abs(r * q).sum(axis=1)
    else:
        big = ((r - q) ** 2).sum(axis=1)
        s = -big
    gone = np.isnan(s)
    return np.where(gone, -np.inf, s), np.where(gone, 0.0, big)


def separated_topk(s, big, k, g):
    """The k best of scores s (ties by position), and whether fp32 scores within g * big of them name the same set: the
    smallest lower bound among the k best lies above the largest upper bound among the rest.  Where every S is alike this is
    'the gap between the k-th and the (k + 1)-th score exceeds 2 g S'."""
    order = np.lexsort((np.arange(len(s)), -s))
    top, rest = order[:k], order[k:]
    if len(top) < k or not np.all(np.isfinite(s[top])):
        return top, False
    if not len(rest):
        return top, True
    return top, bool((s[top] - g * big[top]).min() > (s[rest] + g * big[rest]).max())


def reference_check(model, pitch, name, got, listed=None, thresholds=None):
    """One call's result against float64 scores of the model's rows.  name: "search" (any route; got = (ids, scores) for the
    model's queries), "search_rows" (listed = its rows), "search_distinct" (got = (ids, scores, labels)), "range_search"
    (thresholds per query).  Returns (errors, pairs checked, pairs skipped for a gap inside the fp32 error)."""
    g, metric = gamma(pitch), model.metric
    errors, checked, skipped = [], 0, 0
    if name == "range_search":
        offsets, rows, _ = got
        for qi in range(len(offsets) - 1):
            s, big = scores64(model.rows, model.queries[qi], metric)
            t = float(np.broadcast_to(thresholds, (len(offsets) - 1,))[qi])
            t = t if metric == "cosine" else -t                       # (L2: squared distance <= t is score >= -t)
            back = set(rows[int(offsets[qi]):int(offsets[qi + 1])].tolist())
            must = set(np.flatnonzero(s - t > g * big).tolist())
            never = set(np.flatnonzero(t - s > g * big).tolist())
            checked += 1
            if must - back:
                errors.append(f"range_search query {qi}: rows {sorted(must - back)[:5]} lie above the threshold and are missing")
            if never & back:
                errors.append(f"range_search query {qi}: rows {sorted(never & back)[:5]} lie below the threshold")
        return errors, checked, skipped
    ids = got[0]
    k = ids.shape[1]
    for qi in range(len(ids)):
        s, big = scores64(model.rows, model.queries[qi], metric)
        where = np.arange(len(s))
        if name == "search_rows":
            where = np.asarray(listed, np.int64)
            s, big = s[where], big[where]
        if name == "search_distinct":
            # a label's bounds are those of its best row: per label the largest lower and the largest upper bound
            lab = model.labels.astype(np.int64)
            key = np.where(lab == LABEL_NONE, -1 - np.arange(len(lab)), lab)     # (a row without a label is one of its own)
            keys, inv = np.unique(key, return_inverse=True)
            live = np.isfinite(s)
            lo = np.full(len(keys), -np.inf)
            hi = np.full(len(keys), -np.inf)
            np.maximum.at(lo, inv[live], (s - g * big)[live])
            np.maximum.at(hi, inv[live], (s + g * big)[live])
            mid = np.full(len(keys), -np.inf)
            np.maximum.at(mid, inv[live], s[live])
            order = np.lexsort((np.arange(len(keys)), -mid))
            top, rest = order[:k], order[k:]
            sure = len(top) == k and np.all(np.isfinite(mid[top])) and (not len(rest) or lo[top].min() > hi[rest].max())
            expect = set(keys[top].tolist())
            back = set(int(key[r]) for r in ids[qi] if r >= 0)
        else:
            top, sure = separated_topk(s, big, k, g)
            expect = set(where[top].tolist())
            back = set(ids[qi].tolist())
        if not sure:
            skipped += 1
            continue
        checked += 1
        if back != expect:
            errors.append(f"{name} query {qi}: {sorted(back)} returned, the float64 top-{k} is {sorted(expect)}")
    return errors, checked, skipped
