"""tests/log_checks.py on the CPU: the references of the counting sort and of the two reduce kernels on hand-written logs whose answers are
written out here, and the builders of the synthetic logs of tests/test_gpu_log_pipeline.py: the run lengths, the live counts and the value
ranges they claim (every integer sum below 2^53) are verified here, before anything runs on a GPU."""
import numpy as np
import pytest

import log_checks as L

NAN = np.nan

# a geometry of the kind Engine.log_geometry() reports (the GPU tests take theirs from the engine; nothing here depends on the numbers being the
# engine's), and a toy one: chunks of 8, two thresholds of 3
LIKE_THE_ENGINE = dict(chunk=4096, rf_bucket_bits=13, stat_bucket_bits=11, scan_threads=256, sort_block=512, max_parts=8192, reduce_span=1 << 17,
                       rf_short_run=4096, stat_short_run=1024, max_entries=1 << 24)
TOY = dict(chunk=8, rf_bucket_bits=2, stat_bucket_bits=1, scan_threads=2, sort_block=2, max_parts=8, reduce_span=16, rf_short_run=3, stat_short_run=3,
           max_entries=1 << 10)


def test_partition_and_field_reduce_of_a_hand_written_log():
    """chunks of 4, partitions of 4 keys; 5 device cells (two of them padding) x 2 bins = 10 keys in 3 partitions; 3 real cells"""
    chunk, bits, parts, nl, rf_keys = 4, 2, 3, 2, 10
    ext = [2, -1, 0, 1, -1]
    keys = np.array([0, 1, 5, 12, 9, 4, 11, 3], dtype=np.uint32)  # 12: the pad key (partition 3); 11: in the last partition, beyond the table
    vals = np.arange(1., 9.)
    assert L.live_mask(keys, None, chunk, bits, parts).tolist() == [True, True, True, False, True, True, True, True]
    assert L.partition_starts(keys, None, chunk, bits, parts).tolist() == [0, 3, 5, 7]
    # key 0 -> cell 2 bin 0, key 1 -> cell 2 bin 1, key 5 -> device cell 2 = cell 0, bin 1, key 4 -> cell 0 bin 0; 9 and 3: padding slots
    assert L.rf_reduce(keys, vals, ext, nl, rf_keys, 6, parts, bits).tolist() == [6., 3., 0., 0., 1., 2.]
    assert L.rf_table_index(keys, ext, nl, rf_keys).tolist() == [4, 5, 1, -1, -1, 0, -1, -1]

    def problem(sorted_keys, sorted_vals, start):
        return L.partition_problem(keys, vals, None, chunk, bits, parts, np.array(sorted_keys, dtype=np.uint32), np.array(sorted_vals), start)

    good_keys, good_vals, good_start = [3, 0, 1, 4, 5, 11, 9, 0], [8., 1., 2., 6., 3., 7., 5., 0.], [0, 3, 5, 7]
    assert problem(good_keys, good_vals, good_start) is None
    # a value in the wrong partition (with its key), a value with another value's key, a wrong start, a lost entry, an entry beyond the end
    assert "values of some partition" in problem([3, 0, 4, 1, 5, 11, 9, 0], [8., 1., 6., 2., 3., 7., 5., 0.], good_start)
    assert "lost the key" in problem([0, 3, 1, 4, 5, 11, 9, 0], good_vals, good_start)
    assert "start differs" in problem(good_keys, good_vals, [0, 2, 5, 7])
    assert "values of some partition" in problem(good_keys, [8., 1., 2., 6., 3., 7., 7., 0.], good_start)
    assert "beyond start" in problem(good_keys[:7] + [12], good_vals, good_start)


def test_statistics_reduce_of_a_hand_written_log_with_open_chunks():
    """chunks of 4, partitions of 2 records, 5 records in 3 partitions; chunks filled 2, 1 and 4, poison behind the fills"""
    chunk, bits, parts, records = 4, 1, 3, 5
    fills = np.array([2, 1, 4], dtype=np.uint32)
    keys = np.array([0, 4, 0, 0, 3, 0, 0, 0, 6, 5, 2, 2], dtype=np.uint32)  # 6: the pad key; 5: in the last partition, beyond the records
    vals = np.array([2., 3., NAN, NAN, .5, NAN, NAN, NAN, 7., 9., 2., 3.])
    assert L.live_mask(keys, fills, chunk, bits, parts).tolist() == [True, True, False, False, True, False, False, False, False, True, True, True]
    assert L.partition_starts(keys, fills, chunk, bits, parts).tolist() == [0, 1, 4, 6]
    want = [[1., 2., 4., 8., 16.], [0.] * 5, [2., 5., 13., 35., 97.], [1., .5, .25, .125, .0625], [1., 3., 9., 27., 81.]]
    assert L.stat_reduce(keys, vals, records, parts, bits, fills, chunk).tolist() == want
    # without the fills the poison is in: that is what it is there for
    assert np.isnan(L.stat_reduce(keys, vals, records, parts, bits)[0]).any()
    # the builder of poison writes exactly these entries
    k, v = L.poison(np.where(np.isnan(vals), 77, keys).astype(np.uint32), np.nan_to_num(vals, nan=5.), fills, chunk)
    assert np.array_equal(k, keys) and np.array_equal(np.isnan(v), np.isnan(vals))


def test_fsum_reference_and_bound():
    index = np.array([2, 0, 2, -1, 2, 0])
    values = np.array([1e16, 3., 1., 5., -1e16, .25])
    total, count, magnitude = L.fsum_by_key(index, values, 4)
    assert total.tolist() == [3.25, 0., 1., 0.] and count.tolist() == [2, 0, 3, 0] and magnitude.tolist() == [3.25, 0., 2e16 + 1, 0.]
    # (n_k - 1) 2^-53 sum|v|; k more units per term for a power k >= 2; a single entry is exact
    assert L.sum_bound(count, magnitude).tolist() == [3.25 * 2.0 ** -53, 0., 2 * (2e16 + 1) * 2.0 ** -53, 0.]
    assert L.sum_bound(np.array([1]), np.array([8.]))[0] == 0. and L.sum_bound(np.array([1]), np.array([8.]), power=3)[0] == 3 * 8. * 2.0 ** -53


def _runs(keys, fills, g, bits, parts):
    return np.diff(L.partition_starts(keys, fills, g["chunk"], bits, parts).astype(np.int64))


@pytest.mark.parametrize("g", [TOY, LIKE_THE_ENGINE], ids=["toy", "like the engine"])
def test_partition_logs_are_what_they_claim(g):
    for bits in (g["rf_bucket_bits"], g["stat_bucket_bits"]):
        for parts in (1, 2, g["scan_threads"] + 1, g["max_parts"]):
            keys, vals, fills = L.uniform_partition_log(g, bits, parts, 3, seed=parts)
            assert keys.size == 3 * g["chunk"] and fills is None and np.unique(vals).size == vals.size and vals.min() == 1.
            pad = min(parts << bits, L.NO_KEY)
            if g is LIKE_THE_ENGINE:
                assert 0.03 < (keys == pad).mean() < 0.08 and 0.03 < (keys > pad).mean() < 0.07 and keys.max() > 1 << 30
                assert abs(int(L.live_mask(keys, None, g["chunk"], bits, parts).sum()) - 0.9 * keys.size) < 0.02 * keys.size
                if parts <= g["scan_threads"] + 1:
                    assert (_runs(keys, None, g, bits, parts) > 0).all()
        parts = 7 * 9 + 1
        for where in ([0], [parts // 2], [parts - 1], list(range(0, parts, 7))):
            keys, vals, _ = L.skewed_partition_log(g, bits, parts, 2, where, seed=3)
            runs = _runs(keys, None, g, bits, parts)
            assert runs.sum() == int(0.9 * keys.size) and set(np.flatnonzero(runs)) <= set(where)
            if g is LIKE_THE_ENGINE:
                assert set(np.flatnonzero(runs)) == set(where)
        assert _runs(L.skewed_partition_log(g, bits, parts, 1, [], seed=4)[0], None, g, bits, parts).sum() == 0
        assert _runs(L.skewed_partition_log(g, bits, parts, 1, [5], seed=4, live=1)[0], None, g, bits, parts).tolist() == [0] * 5 + [1] + [0] * (parts - 6)
        keys, vals, fills = L.filled_log(g, bits, parts, parts << bits, seed=5)
        c = g["chunk"]
        assert set(fills.tolist()) >= {0, 1, 2, 3, 4, 5, g["sort_block"] - 1, c - 1, c} and fills.max() == c and keys.size == fills.size * c
        gone = np.isnan(vals)
        assert gone.sum() == keys.size - int(fills.sum()) and np.all(keys[gone] == 0)
        assert np.array_equal(gone.reshape(-1, c), np.arange(c)[None, :] >= fills[:, None].astype(np.int64))


@pytest.mark.parametrize("kind,parts,table_keys", [("rf", 13, 105552), ("rf", 1, 2000), ("rf", 40, 40 * 8192 - 3000), ("stat", 9, 16640), ("stat", 33, 33 * 2048 - 7)])
def test_reduce_logs_are_what_they_claim(kind, parts, table_keys):
    """the families of the reduce tests on a geometry like the engine's: run lengths, live totals, value ranges, and every integer sum < 2^53"""
    g = LIKE_THE_ENGINE
    bits, short, span, chunk = g[kind + "_bucket_bits"], g[kind + "_short_run"], g["reduce_span"], g["chunk"]
    seen = set()
    for name, (keys, vals, fills) in L.reduce_logs(g, kind, parts, table_keys):
        seen.add(name)
        assert keys.size % chunk == 0 and 0 < keys.size <= g["max_entries"] and keys.dtype == np.uint32 and vals.dtype == np.float64
        runs = _runs(keys, fills, g, bits, parts)
        live = L.live_mask(keys, fills, chunk, bits, parts)
        assert np.all(vals[live] == np.floor(vals[live])) and vals[live].min() >= 1.
        if kind == "rf":
            assert vals[live].max() <= L.RF_VALUE_MAX
            table = L.rf_reduce(keys, vals, np.arange(table_keys), 1, table_keys, table_keys, parts, bits)
            assert table.max() < L.EXACT
        else:
            busiest = np.bincount(keys[live & (keys < table_keys)].astype(np.int64)).max()
            assert vals[live].max() <= L.STAT_WEIGHT_MAX and (busiest <= L.STAT_RECORD_ENTRIES or name == "three spans on one key")
            acc = L.stat_reduce(keys, vals, table_keys, parts, bits, fills, chunk)
            assert acc.max() <= float(1 << 52) and np.all(acc == np.floor(acc)) and not np.isnan(acc).any()
            assert acc[:, 0].sum() == (live & (keys < table_keys)).sum()
        if name == "coverage":
            assert np.array_equal(np.sort(keys[live]), np.arange(parts << bits)) and np.all(runs == 1 << bits)
        elif name.startswith("run of"):
            entries = int(name.split()[2])
            assert entries in (short - 1, short, short + 1) and sorted(runs[runs > 0].tolist()) == [entries]
            inside = keys[live & (keys < table_keys)]
            assert np.unique(inside).size == (1 if "one key" in name else min(entries, inside.size)) and inside.size > 0
            assert "one key" not in name or inside.size == entries
        elif name == "three spans on one key":
            assert runs.max() == 3 * span == runs.sum() and np.unique(keys[live]).size == 1 and keys[live][0] < table_keys
        elif name.endswith("live entries"):
            assert runs.sum() == int(name.split()[0]) and runs.sum() in (span - 1, span, span + 1)
        elif name.startswith("span boundary"):
            first = np.flatnonzero(runs)[0]
            assert runs[first] + runs[first + 1] == span and np.all(runs[first + 2:first + 2 + 24] == 0) and runs[first + 2 + 24] > 0 and runs[-1] > 0
        elif name == "open and short chunks":
            assert fills is not None and np.isnan(vals).sum() == keys.size - int(fills.sum())
        if fills is None:
            assert not np.isnan(vals).any()
    want = {"coverage", "three spans on one key", "mixed"} | {f"{t} live entries" for t in (span - 1, span, span + 1)}
    want |= {f"run of {e} {how}" for e in (short - 1, short, short + 1) for how in ("on one key", "over the keys")}
    want |= {"span boundary in a streak of empty partitions"} if parts >= 28 else set()
    want |= {"open and short chunks"} if kind == "stat" else set()
    assert seen == want
    # the non-integer pass: positive, not integers, runs on both sides of the threshold and a cut by a span boundary
    keys, vals, fills = L.non_integer_log(g, kind, parts, table_keys)
    runs = _runs(keys, fills, g, bits, parts)
    assert vals.min() > 0. and (vals != np.floor(vals)).mean() > 0.99 and runs.sum() > span and runs.max() >= short
