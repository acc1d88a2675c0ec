"""The ranking kernels by themselves: ``merge_kernel`` (register merge, threshold + LDS sort, list walk), ``kth_score_kernel``
(``block_kth_threshold``) and the radix select chain, launched by tests/kernel_harness on key arrays built here -- the hard
inputs a search on random vectors reaches by luck or not at all (ties across the k-th boundary, list counts around the
register paths' limits, clamped list counts, absent keys, every boundary value of k).

Reference for everything: numpy on uint64.  A key is ``(f2ord(score) << 32) | ~row``, 0 = absent; the expected output of a
merge or a select is "gather the query's keys by the strides, drop zeros, sort descending, take k".  Integer arithmetic, so
every comparison is ``array_equal`` on keys, ids and the BIT PATTERNS of scores and thresholds.  Padding when fewer than k keys
exist: key 0, id -1, score +0.0, out_kth -inf.

Preconditions of the kernels that the harness respects: every input list is sorted descending with its absent
keys at the tail; keys are unique; scores are not NaN."""
import zlib

import numpy as np
import pytest

import rank_harness as H

U32, U64 = np.uint32, np.uint64
NEG_INF_BITS = 0xFF800000
ALL_K = [1, 2, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 150, 300, 511, 512, 513, 963, 964, 2048]
FAR = 1_000_000_000  # a candidate count far above P
MAX_KEYS_PER_QUERY = 60_000  # (512 lists of 2 048 slots are filled partly: the walk is per list, the reference's sort per key)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# --------------------------------------------------------------------------- #
# CPU: the reference's own tools
# --------------------------------------------------------------------------- #
def test_f2ord_orders_floats_as_numpy_sort_does_and_round_trips():
    rng = _rng("f2ord")
    bits = rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(U32)
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000], U32)
    bits = np.concatenate([bits, edge])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]  # every finite float, both zeros, both infinities
    o = H.f2ord(x)
    assert np.array_equal(H.ord2f(o).view(U32), x.view(U32))  # round trip, bit for bit
    assert np.all(o != 0)  # 0 is left for "absent"
    by_ord = x[np.argsort(o, kind="stable")]
    assert np.array_equal(by_ord, np.sort(x))  # the same order as numpy's on the values ...
    # ... and one step finer: -0.0 strictly below +0.0 (numpy calls them equal)
    assert H.f2ord(np.float32(-0.0))[0] + 1 == H.f2ord(np.float32(0.0))[0] == 0x80000000
    xs = np.sort(x)
    strictly = xs[1:] > xs[:-1]
    os_ = np.sort(o)
    assert np.all((os_[1:] > os_[:-1])[strictly])
    assert H.f2ord(np.float32(-np.inf))[0] == 0x007FFFFF and H.f2ord(np.float32(np.inf))[0] == 0xFF800000
    # the inverse is defined on every bit pattern (thresholds are prefixes, not scores)
    u = H.ord2f(bits).view(U32)
    back = np.where(u >> U32(31) != 0, ~u, u ^ U32(0x80000000)).astype(U32)
    assert np.array_equal(back, bits)


def test_harness_is_built_from_the_product_headers_and_defines_no_kernel():
    src = H.SOURCE.read_text()
    assert '#include "kernels_common.h"' in src and '#include "kernels_merge_select.h"' in src
    assert "__global__" not in src
    mk = (H.ROOT / "wdbx-py_amd" / "csrc" / "Makefile").read_text()
    assert "rank_harness.hip" in mk and "librank_harness.so" in mk
    # the library's own launch goes through the same helpers the harness calls
    host = (H.ROOT / "wdbx-py_amd" / "csrc" / "host_index.h").read_text()
    for helper in ("merge_launch_for", "enqueue_merge", "enqueue_kth", "enqueue_radix_select", "enqueue_sort_out"):
        assert helper + "(" in src and helper + "(" in host, helper
    for kernel in ("merge_kernel<", "kth_score_kernel,", "radix_hist_kernel,", "sort_out_kernel,"):
        assert kernel not in host, f"{kernel} launched in line in host_index.h"


# --------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------- #
def _expected(top, k, metric=H.METRIC_COSINE, row_base=0, idx_base=0):
    """top: the query's best keys, descending, at most k -> (keys, idx, score bits, kth bits) as the kernels write them."""
    top = np.asarray(top, U64)
    m = top.size
    keys, idx, score = np.zeros(k, U64), np.full(k, -1, np.int64), np.zeros(k, np.float32)
    row = H.key_row(top)
    out_row = (row + U64(row_base)) & U64(0xFFFFFFFF)
    keys[:m] = (top & U64(0xFFFFFFFF00000000)) | ((~out_row) & U64(0xFFFFFFFF))
    idx[:m] = row.astype(np.int64) + np.int64(idx_base)
    s = H.ord2f(H.key_ord(top))
    if metric == H.METRIC_L2:
        s = (-s) + np.float32(0.0)
    score[:m] = s
    kth = int(H.ord2f(H.key_ord(top[k - 1: k])).view(U32)[0]) if m >= k else NEG_INF_BITS
    return keys, idx, score.view(U32), kth


def _top(keys, k):
    keys = np.asarray(keys, U64)
    keys = keys[keys != 0]
    return np.sort(keys)[::-1][:k]


class Case:
    """nq queries' lists laid out in one array by (q_stride, i_stride, p_stride)."""

    def __init__(self, nq, P, list_len, layout, pad=0):
        self.nq, self.P, self.list_len, self.layout = nq, P, list_len, layout
        if layout == "interleaved":      # [q][i][p]: the scans' transposed partial lists, the candidates
            self.ps, self.is_, self.qs = 1, P, P * list_len + pad
            size = nq * self.qs
        elif layout == "listmajor":      # [q][p][i], lists apart by more than their length
            self.ps, self.is_ = list_len + pad, 1
            self.qs = P * self.ps + pad
            size = nq * self.qs
        elif layout == "group":          # [p][q][i]: the shard group's gathered lists
            self.ps, self.is_, self.qs = nq * list_len, 1, list_len
            size = P * self.ps
        else:
            raise ValueError(layout)
        self.arr = np.zeros(max(size, 1) + pad, U64)
        pp, ii = np.meshgrid(np.arange(P, dtype=np.int64), np.arange(list_len, dtype=np.int64), indexing="ij")
        self._off = pp * self.ps + ii * self.is_  # [P, list_len]

    def put(self, q, lists):
        """lists: [P, list_len] uint64, every row sorted descending, zeros at the tail."""
        assert lists.shape == (self.P, self.list_len)
        self.arr[q * self.qs + self._off] = lists

    def gather(self, q, p_used):
        return self.arr[q * self.qs + self._off[:p_used]].ravel()


def _deal(rng, keys, P, list_len):
    """Spread keys (unique, non-zero) over P lists of list_len slots at random; each list sorted descending, zeros behind."""
    keys = np.asarray(keys, U64)
    assert keys.size <= P * list_len and np.unique(keys).size == keys.size and np.all(keys != 0)
    lists = np.zeros((P, list_len), U64)
    if keys.size == 0:
        return lists
    slots = rng.choice(P * list_len, keys.size, replace=False)
    lid = slots // list_len
    order = np.lexsort((~keys, lid))  # by list, then key descending
    lid, keys = lid[order], keys[order]
    start = np.searchsorted(lid, lid, side="left")
    lists[lid, np.arange(keys.size) - start] = keys
    return lists


def _random_keys(rng, n, row_hi=1 << 20, scale=1.0):
    """n unique keys with normal scores (duplicated SCORES are likely for large n: rows break them)."""
    sc = (rng.standard_normal(n) * scale).astype(np.float32)
    rows = rng.choice(max(row_hi, 2 * n), n, replace=False)
    return H.make_keys(H.f2ord(sc), rows)


def _variants(k):
    """(lds_lists, no_fast): the register-list instance exists up to k = 128; option lds_lists forces the LDS one."""
    v = [(0, 0), (0, 1)]
    if k <= 128:
        assert H.merge_geometry(k, 0)[2] and not H.merge_geometry(k, 1)[2]
        v += [(1, 0), (1, 1)]
    else:
        assert not H.merge_geometry(k, 0)[2]
    return v


def _run_and_check(case, k, P_dev=None, metric=H.METRIC_COSINE, row_base=0, idx_base=0, what=""):
    """Every variant of the launch against the reference (and so against each other)."""
    nq, P = case.nq, case.P
    exp = []
    for q in range(nq):
        p_used = P if P_dev is None else min(int(P_dev[q]), P)
        exp.append(_expected(_top(case.gather(q, p_used), k), k, metric, row_base, idx_base))
    e_keys, e_idx = np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])
    e_score, e_kth = np.stack([e[2] for e in exp]), np.array([e[3] for e in exp], U32)
    e_over = np.array([0 if P_dev is None else int(int(P_dev[q]) > P) for q in range(nq)], U32)
    first = None
    for lds_lists, no_fast in _variants(k):
        got = H.merge(case.arr, nq, k, P, case.list_len, case.qs, case.is_, case.ps, metric, row_base, idx_base, P_dev=P_dev,
                      no_fast=no_fast, lds_lists=lds_lists)
        tag = f"{what} k={k} P={P} list_len={case.list_len} {case.layout} lds_lists={lds_lists} no_fast={no_fast}"
        for q in range(nq):
            bad = np.nonzero(got["keys"][q] != e_keys[q])[0]
            assert bad.size == 0, (f"{tag} query {q}: {bad.size} of {k} keys differ, first at rank {bad[0]}: "
                                   f"got {int(got['keys'][q][bad[0]]):#018x} expected {int(e_keys[q][bad[0]]):#018x}; "
                                   f"distinct keys returned {np.unique(got['keys'][q]).size}")
        assert np.array_equal(got["idx"], e_idx), tag
        assert np.array_equal(got["score"], e_score), tag
        assert np.array_equal(got["kth"], e_kth), tag
        assert np.array_equal(got["over"], e_over), tag
        if first is None:
            first = got
        else:
            for name in ("keys", "idx", "score", "kth", "over"):
                assert np.array_equal(first[name], got[name]), (tag, name)


def _p_dev_for(P):
    """One query each: no list, one, all but one, all, one too many, far too many (both clamped, over_out = 1)."""
    return np.array([P, 0, 1, max(P - 1, 0), P + 1, FAR], dtype=np.int64).astype(U32)


def _fill_random(rng, case, fill):
    """Every list of every query filled (so a list past P_dev holds keys that must NOT be read), contents differ per query."""
    for q in range(case.nq):
        total = case.P * case.list_len
        n = min(total if fill[q % len(fill)] >= 1.0 else int(total * fill[q % len(fill)]), MAX_KEYS_PER_QUERY)
        case.put(q, _deal(rng, _random_keys(rng, n), case.P, case.list_len))


def _layouts(i):
    return ["interleaved", "listmajor", "group"][i % 3]


# --------------------------------------------------------------------------- #
# merge_kernel
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_merge_of_sorted_lists(k):
    """P sorted lists of k keys (the scans' partial lists): every P of the matrix, P * k on both sides of 2 048 (two keys per
    thread or eight) and of 8 192 (registers or the list walk), all layouts, q_stride larger than the data, per-query list
    counts from 0 to far above P."""
    ps = {1, 2, 63, 64, 65, 512}
    for limit in (2048, 8192):
        ps |= {max(1, limit // k), limit // k + 1}
    for n, P in enumerate(sorted(ps)):
        rng = _rng("sorted", k, P)
        big = P * k > 40_000
        for layout in ([_layouts(n)] if big else ["interleaved", "listmajor", "group"]):
            case = Case(6, P, k, layout, pad=0 if layout == "group" else 7)
            _fill_random(rng, case, fill=[1.0, 1.0, 0.6, 1.0, 1.0, 0.3])
            _run_and_check(case, k, P_dev=_p_dev_for(P), what="sorted lists")
            if not big:
                _run_and_check(case, k, P_dev=None, what="sorted lists, no P_dev")


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_merge_of_unsorted_candidates(k):
    """list_len = 1: P candidates per query in any order (re-scored candidates, sampled lower bounds)."""
    for P in (1, 2, 63, 64, 65, 512, 2048, 2049, 8192, 8193):
        rng = _rng("cand", k, P)
        for layout, pad in (("interleaved", 0), ("interleaved", 11), ("listmajor", 2)):
            case = Case(6, P, 1, layout, pad=pad)
            _fill_random(rng, case, fill=[1.0, 1.0, 0.5, 1.0, 1.0, 1.0])
            _run_and_check(case, k, P_dev=_p_dev_for(P), what="candidates")
        # i_stride is never used with one entry per list: the library passes 0
        case = Case(3, P, 1, "interleaved", pad=3)
        case.is_ = 0
        _fill_random(rng, case, fill=[1.0, 0.9, 1.0])
        _run_and_check(case, k, P_dev=None, what="candidates, i_stride 0")


@pytest.mark.gpu
@pytest.mark.parametrize("k_out", ALL_K)
def test_merge_of_short_lists_into_a_longer_one(k_out):
    """The shard group's final merge: S lists of list_len < k_out keys into k_out (host_group.h), S * list_len below, at and
    above k_out."""
    shapes = {(8, max(1, k_out // 4)), (2, max(1, (k_out + 1) // 2)), (3, max(1, k_out - 1)), (8, max(1, k_out // 8)),
              (64, max(1, k_out // 16)), (5, max(1, k_out // 7))}
    for S, list_len in sorted(shapes):
        rng = _rng("short", k_out, S, list_len)
        for layout in ("group", "listmajor"):
            case = Case(6, S, list_len, layout, pad=0 if layout == "group" else 5)
            _fill_random(rng, case, fill=[1.0, 1.0, 0.7, 1.0, 1.0, 1.0])
            _run_and_check(case, k_out, P_dev=_p_dev_for(S), what="short lists")
            _run_and_check(case, k_out, P_dev=None, what="short lists, no P_dev")


def _tie_pool(rng, k, T, mode, below):
    """Keys whose k-th best lies inside a group of T keys that are tied (``exact``: one score) or nearly tied (``near``: scores
    that differ only below bit 8 of the ordered score, all inside one 2^8-aligned block); ``outside``: the k-th best lies in a
    small group one 2^8 block ABOVE the T keys, which therefore do not reach the threshold.  Distinct rows everywhere."""
    base = int(H.f2ord(np.float32(0.73))[0]) & ~0xFF
    rows = rng.permutation(k + T + below + 64)
    if mode == "outside":
        above_n = max(0, k - 3)
        mid = base + 256 + rng.integers(0, 256, 6)            # the k-th best is one of these six
        group = base + rng.integers(0, 256, T)                # up to 255 units below the threshold's block
        ords = np.concatenate([base + 4096 + rng.integers(0, 1 << 20, above_n), mid, group, base - 4096 - rng.integers(0, 1 << 20, below)])
    else:
        above_n = 0 if T >= 2 * k else max(0, k - max(1, T // 2))  # 0 < k - above_n <= T: the boundary falls inside the group
        assert above_n < k <= above_n + T
        group = np.full(T, base + 77) if mode == "exact" else base + rng.integers(0, 256, T)
        ords = np.concatenate([base + 4096 + rng.integers(0, 1 << 20, above_n), group, base - 4096 - rng.integers(0, 1 << 20, below)])
    return H.make_keys(ords.astype(U32), rows[: ords.size])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_merge_with_ties_across_the_kth_boundary(k):
    """T keys tied at the k-th score with T up to 8 192: more than 1 024 keys at or above the threshold send the medium-k path
    (k 17 .. 512) to the list walk, whose per-wave lists share the LDS the keys were compacted into."""
    for T in sorted({k, 1023, 1024, 1025, 1200, 4096, 8192}):
        for mode in ("exact", "near", "outside"):
            # unsorted candidates: every key a list of its own; P just large enough, and once the register paths' limit
            shapes = []
            need = k + T + 70
            for P in sorted({min(8192, max(need, 64)), 8192}):
                if need <= P:
                    shapes.append((P, 1, "interleaved"))
            if not shapes:
                shapes.append((need, 1, "interleaved"))  # does not fit the registers: the list walk by size
            # sorted lists of k keys holding the same pool, inside the registers where they fit
            P_lists = -(-need // k) + 1
            shapes.append((P_lists, k, "interleaved" if T % 2 else "listmajor"))
            if P_lists * k > 8192 and 8192 // k >= 2 and (8192 // k) * k >= k + T:
                shapes.append((8192 // k, k, "group"))
            for P, list_len, layout in shapes:
                rng = _rng("ties", k, T, mode, P, list_len)
                case = Case(3, P, list_len, layout, pad=0 if layout == "group" else 3)
                for q in range(3):
                    room = P * list_len - (k + T + 6)
                    below = int(min(room, [0, 40, room][q])) if room > 0 else 0
                    case.put(q, _deal(rng, _tie_pool(rng, k, T, mode, below), P, list_len))
                _run_and_check(case, k, P_dev=None, what=f"ties T={T} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_merge_with_few_or_no_keys(k):
    """Fewer than k present keys (zeros at the lists' tails), no key at all, exactly k - 1, k and k + 1 keys."""
    for P, list_len, layout in ((4, k, "interleaved"), (9, k, "listmajor"), (max(k + 1, 70), 1, "interleaved"), (3, max(1, (k + 2) // 3 + 1), "group")):
        rng = _rng("few", k, P, list_len)
        counts = [0, max(k - 1, 0), k, k + 1, 1, k // 2]
        case = Case(len(counts), P, list_len, layout, pad=0 if layout == "group" else 4)
        for q, n in enumerate(counts):
            n = min(n, P * list_len)
            case.put(q, _deal(rng, _random_keys(rng, n), P, list_len))
        _run_and_check(case, k, P_dev=None, what="few keys")
        _run_and_check(case, k, P_dev=np.array([P, P, P + 1, P, 0, FAR], U32), what="few keys, P_dev")


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38,
                    0.5, -0.5, 1e-30, -1e-30], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 16, 17, 64, 128, 129, 300, 512, 513, 964, 2048])
@pytest.mark.parametrize("metric", [H.METRIC_COSINE, H.METRIC_L2])
def test_merge_of_special_scores_and_rows(k, metric):
    """Negative scores, both zeros (-0.0 ranks below +0.0; an L2 score is written as -s + 0.0, never -0.0), infinities,
    denormals; rows 0 and 2^32 - 2; row_base / idx_base added on the way out."""
    for P, list_len, layout in ((40, 1, "interleaved"), (5000, 1, "interleaved"), (6, k, "listmajor"), (70, k, "interleaved")):
        rng = _rng("special", k, metric, P, list_len)
        case = Case(4, P, list_len, layout, pad=2)
        for q in range(4):
            n = min(P * list_len, [SPECIAL.size * 2, 37, P * list_len, k + 9][q])
            sc = np.concatenate([np.repeat(SPECIAL, 2), (rng.standard_normal(max(n, 1)) * 1e-3).astype(np.float32)])[:n]
            rng.shuffle(sc)
            rows = np.concatenate([[0, (1 << 32) - 2], rng.choice((1 << 32) - 4, max(n, 2), replace=False) + 1])[:n]
            case.put(q, _deal(rng, H.make_keys(H.f2ord(sc), rows), P, list_len))
        _run_and_check(case, k, metric=metric, what="special")
        _run_and_check(case, k, metric=metric, row_base=123_456, idx_base=9_000_000_000, P_dev=np.array([P, P + 1, P - 1, FAR], U32),
                       what="special, bases")
        _run_and_check(case, k, metric=metric, row_base=5, idx_base=-3, what="special, wrap")  # (2^32 - 2) + 5 wraps in out_keys


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 17, 100, 128, 129, 512, 513, 964, 2048])
def test_merge_skips_queries_at_or_below_over_cap(k):
    """only_if_over: a repair merge runs for the queries whose counter exceeds over_cap and leaves every output of the others
    as it found it."""
    P, cap = 33, 1000
    rng = _rng("skip", k)
    case = Case(5, P, k, "interleaved", pad=1)
    _fill_random(rng, case, fill=[1.0])
    over = np.array([cap + 1, cap, 0, FAR, cap - 1], U32)
    for lds_lists, no_fast in _variants(k):
        got = H.merge(case.arr, 5, k, P, k, case.qs, case.is_, case.ps, only_if_over=over, over_cap=cap, P_dev=np.full(5, P + 1, U32),
                      no_fast=no_fast, lds_lists=lds_lists)
        for q in range(5):
            if over[q] > cap:
                e = _expected(_top(case.gather(q, P), k), k)
                assert np.array_equal(got["keys"][q], e[0]) and np.array_equal(got["idx"][q], e[1])
                assert np.array_equal(got["score"][q], e[2]) and got["kth"][q] == e[3] and got["over"][q] == 1
            else:
                assert np.all(got["keys"][q] == U64(H.SENT_KEY)) and np.all(got["idx"][q] == H.SENT_IDX)
                assert np.all(got["score"][q] == H.SENT_F32) and got["kth"][q] == H.SENT_F32 and got["over"][q] == H.SENT_U32


@pytest.mark.gpu
def test_merge_geometry_is_the_librarys():
    """What the harness launches is what merge_launch_for says: 16 waves (the register paths' condition) up to k = 963."""
    for k in ALL_K:
        waves, lds, reg = H.merge_geometry(k)
        assert waves == (16 if k <= 963 else 131072 // (8 * k) - 1) and reg == (k <= 128)
        assert lds >= (waves + 1) * k * 8 and (lds >= 8192 or not 16 < k <= 512) and lds <= 160 * 1024


# --------------------------------------------------------------------------- #
# kth_score_kernel / block_kth_threshold
# --------------------------------------------------------------------------- #
def _ord_of_bits(bits):
    bits = int(bits)
    return bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)


def _kth_value_sets(rng, n):
    """Present score halves of six queries (0 = absent entry)."""
    rnd = H.f2ord(rng.standard_normal(n).astype(np.float32))
    a, b = (int(x) for x in H.f2ord(np.array([0.25, -3.0], np.float32)))
    base = int(H.f2ord(np.float32(0.61))[0]) & ~0xFF
    top = int(H.f2ord(np.float32(0.5))[0])  # 0xBF000000; without its top bit: the ordered form of a negative float
    sets = [rnd,
            np.full(n, a, U32),
            np.where(rng.random(n) < 0.5, a, b).astype(U32),
            (base + rng.integers(0, 256, n)).astype(U32),
            np.where(rng.random(n) < 0.5, top, top ^ 0x80000000).astype(U32),
            np.where(rng.random(n) < 0.35, 0, rnd).astype(U32)]
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000, 16 * 1024 - 1, 16 * 1024])
def test_kth_threshold_contract(n):
    """In ordered-integer units, with v the present score halves: fewer than k present -> -inf; else count(v >= t) >= k and
    count(v >= t + 256) < k -- the search keeps the largest prefix (bits 31 .. 8) with at least k values at or above it."""
    assert n <= H.KTH_MAX_N
    rng = _rng("kth", n)
    sets = _kth_value_sets(rng, n)
    nq, qs = len(sets), n + 5
    keys = np.zeros(nq * qs, U64)
    for q, v in enumerate(sets):
        rows = rng.permutation(n)
        keys[q * qs: q * qs + n] = np.where(v != 0, H.make_keys(v, rows), U64(0))
        keys[q * qs + n: (q + 1) * qs] = H.make_keys(np.full(5, 0xFFFFFFF0, U32), np.arange(5))  # beyond n: must not be read
    ks = sorted({1, 2, 3, max(1, n // 2), max(1, n - 1), n, n + 1, max(1, n // 3), min(n, 100), min(n, 2048)})
    for k in ks:
        out = H.kth(keys, n, qs, nq, k)
        for q, v in enumerate(sets):
            present = v[v != 0].astype(np.int64)
            if present.size < k:
                assert out[q] == NEG_INF_BITS, (n, k, q)
                continue
            t = _ord_of_bits(out[q])
            at, above = int(np.count_nonzero(present >= t)), int(np.count_nonzero(present >= t + 256))
            assert at >= k and above < k, (n, k, q, hex(t), at, above)


# --------------------------------------------------------------------------- #
# the radix select chain
# --------------------------------------------------------------------------- #
def _check_select(keys, k, what, alt=None, count=0, cap=0, **kw):
    if alt is None:
        src = keys
    else:
        src = alt if count > cap else keys[:count]
    got = H.select(keys, k, alt=alt, count=count, cap=cap, **kw)
    valid = int(np.count_nonzero(np.asarray(src, U64) != 0))
    e_keys, e_idx, e_score, e_kth = _expected(_top(src, k), k, kw.get("metric", H.METRIC_COSINE), kw.get("row_base", 0), kw.get("idx_base", 0))
    assert got["total"] == valid and got["out_count"] == min(valid, k), (what, got["total"], got["out_count"], valid)
    bad = np.nonzero(got["keys"] != e_keys)[0]
    assert bad.size == 0, (what, k, bad.size, int(bad[0]))
    assert np.array_equal(got["idx"], e_idx) and np.array_equal(got["score"], e_score), (what, k)
    assert got["kth"][0] == e_kth, (what, k)


def _select_key_sets(rng, n):
    out = {"random": _random_keys(rng, n, scale=0.1)}
    if n >= 4:
        mixed = out["random"].copy()
        mixed[rng.random(n) < 0.3] = 0
        out["absent mixed in"] = mixed
        # one score for a large group around every k-th boundary of the test, rows distinct
        ords = np.concatenate([np.full(n - n // 4, H.f2ord(np.float32(0.4))[0], U32), H.f2ord((rng.standard_normal(n // 4) * 0.08).astype(np.float32))])
        out["tie group"] = H.make_keys(ords, rng.permutation(n) + 17)
    if n <= 256:
        out["top seven bytes shared"] = U64(0xBF12345600ABCD00) + rng.permutation(256)[:n].astype(U64)
    if n <= 255:
        out["top byte only"] = ((rng.permutation(255)[:n].astype(U64) + U64(1)) << U64(56)) | U64(0x0012345600ABCDEF)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_001])
def test_radix_select_chain(n):
    rng = _rng("select", n)
    for name, keys in _select_key_sets(rng, n).items():
        for k in (200, 1000, 2048):
            _check_select(keys, k, f"{name} n={n}")
        _check_select(keys, 200, f"{name} n={n} one workgroup", grid=1)
        _check_select(keys, 1000, f"{name} n={n} L2 + bases", metric=H.METRIC_L2, row_base=77, idx_base=1 << 40)


@pytest.mark.gpu
def test_radix_select_chain_on_three_million_keys():
    n = 3_000_001
    rng = _rng("select", n)
    sc = (rng.standard_normal(n) * 0.1).astype(np.float32)
    sc[:1500] = np.float32(0.93)                # 1 500 tied at the very top: k = 200 and 1 000 cut through them ...
    sc[rng.random(n) < 0.2] = np.float32(0.36)  # ... and 600 k tied 3.6 sigma out, a few hundred ranks on: k = 2 048 cuts through these
    keys = H.make_keys(H.f2ord(sc), rng.permutation(n))
    keys[rng.random(n) < 0.05] = 0
    for k in (200, 1000, 2048):
        _check_select(keys, k, "3 M keys")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [200, 2048])
def test_radix_select_reads_the_source_chosen_on_the_device(k):
    """select_source_kernel: the candidates when their count fits the buffer, else the key-per-row dump; the fixed keys / n
    arguments of the chain are ignored then."""
    rng = _rng("src", k)
    cap = 5000
    cand = _random_keys(rng, cap, scale=0.1)
    dump = _random_keys(rng, 70_001, row_hi=1 << 24, scale=0.1)
    dump[rng.random(dump.size) < 0.1] = 0
    for count in (0, 1, k - 1, k, 4999, 5000):
        _check_select(cand, k, f"candidates count={count}", alt=dump, count=count, cap=cap)
    for count in (5001, 1 << 31):
        _check_select(cand, k, f"dump count={count}", alt=dump, count=count, cap=cap)
