"""Plain numpy references of the counting sort and the reduce kernels behind the radiation-field log and the statistics log
(skirt9_amd/csrc/pmc_log.inc: rfHistKernel, rfScanKernel, rfScatterKernel, rfReduceKernel, statReduceKernel), and the builders of the
synthetic logs that tests/test_gpu_log_pipeline.py sends through them (include/pmc_tuning.h: pmc_tune_log_partition, pmc_tune_rf_log_flush,
pmc_tune_stat_log_flush).  tests/test_log_checks.py checks both on the CPU.

A log is a sequence of chunks of `chunk` (key, value) entries; `fills` (or None: all full) says how many entries of every chunk are there.
A counting sort and a sum have an exact reference: the values of the integer logs are integer-valued doubles whose sums stay below 2^53, so
every sum is exact in any order and the kernels' results are compared with np.array_equal.

Every builder takes the geometry `g` of Engine.log_geometry() (a dict) and hard-codes none of the kernels' constants.
"""
import math

import numpy as np

NO_KEY = 0xFFFFFFFF
RF_VALUE_MAX = 1 << 20    # integer values of the radiation-field logs: [1, 2^20]; 2^24 entries at most: sums <= 2^44
STAT_WEIGHT_MAX = 1 << 10  # integer weights of the statistics logs: [1, 2^10] with at most 2^12 entries per record: sum of w^4 <= 2^52
STAT_RECORD_ENTRIES = 1 << 12
EXACT = float(1 << 53)
U = 2.0 ** -53  # unit roundoff of a double


def live_mask(keys, fills, chunk, bits, num_parts):
    """entries that are there (below their chunk's fill) and whose partition, key >> bits, is one of the num_parts"""
    keys = np.asarray(keys, dtype=np.uint32)
    there = np.ones(keys.size, dtype=bool)
    if fills is not None:
        there = (np.arange(keys.size) % chunk) < np.repeat(np.asarray(fills, dtype=np.int64), chunk)
    return there & ((keys >> np.uint32(bits)).astype(np.int64) < num_parts)


def partition_starts(keys, fills, chunk, bits, num_parts):
    """start[0 .. num_parts]: the exclusive prefix of the live entries per partition"""
    live = live_mask(keys, fills, chunk, bits, num_parts)
    counts = np.bincount((keys[live] >> np.uint32(bits)).astype(np.int64), minlength=num_parts)
    return np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)


def partition_problem(keys, vals, fills, chunk, bits, num_parts, sorted_keys, sorted_vals, start):
    """None if (sorted_keys, sorted_vals, start) is a partition of the log, else what is wrong.  The values of the log must be unique (the
    entry's own index): then partition b of the output must hold exactly the live values of partition b, each with the key it came with,
    and nothing is live beyond start[num_parts] (those places were zeroed before the sort and must still hold zeros)."""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.float64)
    live = live_mask(keys, fills, chunk, bits, num_parts)
    assert np.unique(vals[live]).size == int(live.sum()), "the values of a partition log must be unique"
    want = partition_starts(keys, fills, chunk, bits, num_parts)
    if not np.array_equal(np.asarray(start, dtype=np.uint64), want):
        bad = np.flatnonzero(np.asarray(start, dtype=np.uint64) != want)
        return f"start differs at {bad.size} of {want.size} places, first at {bad[0]}: {start[bad[0]]} for {want[bad[0]]}"
    total = int(want[-1])
    # the live entries ordered by (partition, value), and the output ordered by value inside every partition of `start`
    part = (keys[live] >> np.uint32(bits)).astype(np.int64)
    order = np.lexsort((vals[live], part))
    want_keys, want_vals = keys[live][order], vals[live][order]
    out_part = np.repeat(np.arange(num_parts), np.diff(want.astype(np.int64)))
    got_keys, got_vals = np.asarray(sorted_keys)[:total], np.asarray(sorted_vals)[:total]
    if np.isnan(got_vals).any():
        return "a value from beyond a chunk's fill has reached the partitioned log"
    order = np.lexsort((got_vals, out_part))
    if not np.array_equal(got_vals[order], want_vals):
        return "the values of some partition are not the live values of that partition"
    if not np.array_equal(got_keys[order], want_keys):
        return "some value has lost the key it came with"
    if np.any(np.asarray(sorted_keys)[total:] != 0) or np.any(np.asarray(sorted_vals).view(np.uint64)[total:] != 0):
        return "something was written beyond start[num_parts]"
    return None


def rf_reduce(keys, vals, ext, num_lambda, rf_keys, table_size, num_parts, bits, fills=None, chunk=None):
    """the table rfReduceKernel adds to zeros: vals[i] at ext[key // nl] * nl + key % nl for the live keys < rf_keys with ext >= 0"""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.float64)
    live = live_mask(keys, fills, chunk, bits, num_parts) & (keys.astype(np.int64) < rf_keys)
    k = keys[live].astype(np.int64)
    cell = np.asarray(ext, dtype=np.int64)[k // num_lambda]
    real = cell >= 0
    table = np.zeros(table_size, dtype=np.float64)
    np.add.at(table, cell[real] * num_lambda + k[real] % num_lambda, vals[live][real])
    return table


def rf_table_index(keys, ext, num_lambda, rf_keys):
    """table index of every key, -1 where it has none"""
    k = np.asarray(keys, dtype=np.int64)
    inside = k < rf_keys
    cell = np.where(inside, np.asarray(ext, dtype=np.int64)[np.where(inside, k // num_lambda, 0)], -1)
    return np.where(cell >= 0, cell * num_lambda + k % num_lambda, -1)


def stat_reduce(keys, vals, records, num_parts, bits, fills=None, chunk=None):
    """[records][5]: count, sums of w, w^2, w^3, w^4 per record over the live keys < records"""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.float64)
    live = live_mask(keys, fills, chunk, bits, num_parts) & (keys.astype(np.int64) < records)
    k, w = keys[live].astype(np.int64), vals[live]
    acc = np.zeros((records, 5), dtype=np.float64)
    p = np.ones_like(w)
    for j in range(5):
        np.add.at(acc[:, j], k, p)
        p = p * w  # ((w w) w) w, as the kernel forms the powers
    return acc


# ---- the non-integer pass.  A kernel adds the n_k values v_i of a key in an order (and, through LDS, a tree) of its own: n_k - 1 additions, each
# with a relative error of at most u = 2^-53 of its own result, and every partial result is at most sum|v_i| (1 + O(n u)) in magnitude.  To first
# order in u (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the bound of recursive summation is the worst over EVERY order
# and every tree of n_k - 1 additions) the computed sum differs from the exact one by at most (n_k - 1) u sum|v_i|.  The reference is math.fsum of
# the same doubles: the exact sum, rounded once.  The second-order terms are below 1e-11 of the bound at n_k <= 2^17.
# Powers: w^k is formed as ((w w) w) w, k - 1 roundings of relative error <= u each; k u per term is allowed for them, which also covers the
# reference's own powers (formed the same way, then summed exactly).  Per key and power k >= 2: bound = (n_k - 1 + k) u sum w^k.
def fsum_by_key(index, values, size):
    """math.fsum of the values per index (index >= 0), and per index the number of entries and the sum of |value|"""
    index, values = np.asarray(index, dtype=np.int64), np.asarray(values, dtype=np.float64)
    keep = index >= 0
    index, values = index[keep], values[keep]
    order = np.argsort(index, kind="stable")
    index, values = index[order], values[order]
    total, count, magnitude = np.zeros(size), np.zeros(size, dtype=np.int64), np.zeros(size)
    edges = np.flatnonzero(np.diff(index)) + 1
    for a, b in zip(np.concatenate(([0], edges)), np.concatenate((edges, [index.size]))):
        if b > a:
            total[index[a]] = math.fsum(values[a:b])
            count[index[a]] = b - a
            magnitude[index[a]] = math.fsum(np.abs(values[a:b]))
    return total, count, magnitude


def sum_bound(count, magnitude, power=1):
    """see above: (n_k - 1) u sum|v| for the kernel's additions, and k u per term for the products of a power k >= 2"""
    return (np.maximum(count - 1, 0) + (power if power > 1 else 0)) * U * magnitude


# ---- builders.  Every builder returns (keys uint32 [n], vals float64 [n], fills or None) with n a multiple of the chunk.
def _pad_key(num_parts, bits):
    return np.uint32(min(num_parts << bits, NO_KEY))


def _finish(keys, g, num_parts, bits, rng=None, values=None, shuffle=True):
    """live keys -> a log in whole chunks: filled up with pad keys, shuffled over the chunks (so that every tile of the sort mixes the
    partitions), values: the entry's index + 1 (unique), or integers drawn from [1, values]"""
    keys = np.asarray(keys, dtype=np.uint32)
    chunk = g["chunk"]
    n = max((keys.size + chunk - 1) // chunk, 1) * chunk
    out = np.full(n, _pad_key(num_parts, bits), dtype=np.uint32)
    out[:keys.size] = keys
    if shuffle and rng is not None:
        out = out[rng.permutation(n)]
    vals = np.arange(1, n + 1, dtype=np.float64) if values is None else rng.integers(1, values + 1, size=n).astype(np.float64)
    return out, vals, None


def uniform_partition_log(g, bits, num_parts, tiles, seed):
    """keys uniform over the partitions (and over the keys of a partition), 5 % pad keys (num_parts << bits), 5 % keys anywhere above that up to
    0xFFFFFFFF; values: the entry's index + 1"""
    rng = np.random.default_rng(seed)
    n = tiles * g["chunk"]
    keys = ((rng.integers(0, num_parts, size=n) << bits) | rng.integers(0, 1 << bits, size=n)).astype(np.uint32)
    kind = rng.random(n)
    pad = int(_pad_key(num_parts, bits))
    keys[kind < 0.05] = pad
    above = (kind >= 0.05) & (kind < 0.10)
    keys[above] = rng.integers(pad, NO_KEY + 1, size=int(above.sum())).astype(np.uint32)
    return keys, np.arange(1, n + 1, dtype=np.float64), None


def skewed_partition_log(g, bits, num_parts, tiles, parts, seed, live=None):
    """every live entry in one of the partitions `parts` (a list), the rest pad keys; live: number of live entries (default 90 % of the log)"""
    rng = np.random.default_rng(seed)
    n = tiles * g["chunk"]
    live = int(0.9 * n) if live is None else live
    parts = np.asarray(parts, dtype=np.int64)
    keys = np.full(n, _pad_key(num_parts, bits), dtype=np.uint32)
    if parts.size and live:
        where = rng.permutation(n)[:live]
        keys[where] = ((parts[rng.integers(0, parts.size, size=live)] << bits) | rng.integers(0, 1 << bits, size=live)).astype(np.uint32)
    return keys, np.arange(1, n + 1, dtype=np.float64), None


def fill_values(g):
    """fills of the chunks of a log with open and short chunks: 0, 1 .. 5 (no multiple of the four keys a lane of rfHistKernel loads at a time,
    and one), one less than the lanes of rfScatterKernel, chunk - 1 and chunk, in mixed order"""
    c = g["chunk"]
    return np.array([c, 3, 0, g["sort_block"] - 1, 5, c - 1, 1, 4, 0, 2, c, c - 1], dtype=np.uint32)


def poison(keys, vals, fills, chunk):
    """what lies beyond a chunk's fill: key 0 and value NaN -- a single entry that leaks poisons a result"""
    gone = (np.arange(keys.size) % chunk) >= np.repeat(np.asarray(fills, dtype=np.int64), chunk)
    keys, vals = keys.copy(), vals.copy()
    keys[gone], vals[gone] = 0, np.nan
    return keys, vals


def filled_log(g, bits, num_parts, key_limit, seed, values=None):
    """a log of len(fill_values) chunks with those fills: keys uniform below key_limit (5 % pad keys), the rest of every chunk poison"""
    rng = np.random.default_rng(seed)
    fills = fill_values(g)
    n = fills.size * g["chunk"]
    keys = rng.integers(0, key_limit, size=n).astype(np.uint32)
    keys[rng.random(n) < 0.05] = _pad_key(num_parts, bits)
    vals = np.arange(1, n + 1, dtype=np.float64) if values is None else rng.integers(1, values + 1, size=n).astype(np.float64)
    keys, vals = poison(keys, vals, fills, g["chunk"])
    return keys, vals, fills


# ---- the logs of the reduce tests, the same families for both reduce kernels
def run_keys(rng, bits, runs, one_key, table_keys):
    """runs: [(partition, entries)]: that many entries in that partition -- all on one key of it (one_key; a key of the table where the
    partition has one) or dealt over its keys in turn from its first, the keys between the table's end and the partition's included"""
    keys = []
    for part, entries in runs:
        size = 1 << bits
        inside = min(max(table_keys - (part << bits), 1), size)
        low = np.full(entries, rng.integers(0, inside), dtype=np.int64) if one_key else np.arange(entries) % size
        keys.append((part << bits) | low)
    return np.concatenate(keys)


def streak_keys(rng, g, bits, num_parts, streak=24):
    """a span boundary inside a streak of `streak` empty partitions: the two partitions before the streak are the first with entries and hold
    exactly reduce_span entries together; the partition behind the streak and the last one hold some more"""
    assert num_parts >= streak + 4
    first = (num_parts - streak) // 2
    span = g["reduce_span"]
    runs = [(first - 2, span // 2), (first - 1, span - span // 2), (first + streak, 777), (num_parts - 1, 1501)]
    return np.concatenate([(p << bits) | rng.integers(0, 1 << bits, size=e) for p, e in runs])


def stat_weight_limit(keys, records):
    """the largest weight 2^j <= STAT_WEIGHT_MAX with which the sum of w^4 over the busiest record of this log stays <= 2^52: STAT_WEIGHT_MAX up to
    STAT_RECORD_ENTRIES entries per record, less beyond (a whole span on one record)"""
    keys = np.asarray(keys, dtype=np.int64)
    keys = keys[keys < records]
    busiest = int(np.bincount(keys).max()) if keys.size else 1
    w = STAT_WEIGHT_MAX
    while busiest * w ** 4 > (1 << 52):
        w //= 2
    return w


FAMILIES = ("coverage", "threshold runs", "span edges", "mixed", "open chunks")


def reduce_logs(g, kind, num_parts, table_keys, families=FAMILIES, seed=1):
    """(name, (keys, vals, fills)) for the logs of one context and one reduce kernel -- kind "rf" (table_keys = rf_keys) or "stat" (table_keys =
    stat_records) -- of the families asked for; integer values: [1, RF_VALUE_MAX], or weights [1, stat_weight_limit].  A generator: the logs
    are large, and a log is built when its turn comes."""
    bits, short, span = g[kind + "_bucket_bits"], g[kind + "_short_run"], g["reduce_span"]
    size = num_parts << bits
    middle, last = num_parts // 2, num_parts - 1
    plans = []  # (family, name, function of a generator that gives the live keys, fills)

    # every key of the table (every mapping, every padding slot) and every key between the table's end and the last partition's
    plans.append(("coverage", "coverage", lambda rng: np.arange(size, dtype=np.uint32), None))
    # runs just below, at and above the short-run threshold, in the first, a middle and the last partition
    for i, entries in enumerate((short - 1, short, short + 1)):
        for one_key in (True, False):
            part = (0, middle, last)[(i + one_key) % 3]
            plans.append(("threshold runs", f"run of {entries} {'on one key' if one_key else 'over the keys'}",
                          lambda rng, part=part, entries=entries, one_key=one_key: run_keys(rng, bits, [(part, entries)], one_key, table_keys), None))
    plans.append(("span edges", "three spans on one key", lambda rng: run_keys(rng, bits, [(middle, 3 * span)], True, table_keys), None))
    for live in (span - 1, span, span + 1):
        plans.append(("span edges", f"{live} live entries", lambda rng, live=live: rng.integers(0, size, size=live), None))
    if num_parts >= 28:
        plans.append(("span edges", "span boundary in a streak of empty partitions", lambda rng: streak_keys(rng, g, bits, num_parts), None))
    plans.append(("mixed", "mixed", lambda rng: mixed_keys(rng, g, kind, num_parts, table_keys), None))
    if kind == "stat":
        plans.append(("open chunks", "open and short chunks", lambda rng: filled_log(g, bits, num_parts, size, seed)[0], fill_values(g)))

    for number, (family, name, live_keys, fills) in enumerate(plans):
        if family not in families:
            continue
        rng = np.random.default_rng([seed, number])
        keys = live_keys(rng)
        if fills is None:
            keys, _, _ = _finish(keys, g, num_parts, bits, rng)
        limit = RF_VALUE_MAX if kind == "rf" else stat_weight_limit(keys, table_keys)
        vals = rng.integers(1, limit + 1, size=keys.size).astype(np.float64)
        if fills is not None:
            keys, vals = poison(keys, vals, fills, g["chunk"])
        yield name, (keys, vals, fills)


def mixed_keys(rng, g, kind, num_parts, table_keys):
    """long and short runs side by side, cut by a span boundary: a span and a bit of keys uniform over the table, a long run on one key of a
    middle partition, a run just above the threshold dealt over the keys of the first"""
    bits, short, span = g[kind + "_bucket_bits"], g[kind + "_short_run"], g["reduce_span"]
    return np.concatenate([rng.integers(0, min(num_parts << bits, table_keys + 100), size=span + 1001),
                           run_keys(rng, bits, [(num_parts // 2, 2 * short + 3)], True, table_keys),
                           run_keys(rng, bits, [(0, short + 1)], False, table_keys)])


def non_integer_log(g, kind, num_parts, table_keys, seed=2):
    """the mixed log with random positive non-integer values of (0, 1000)"""
    rng = np.random.default_rng(seed)
    bits = g[kind + "_bucket_bits"]
    keys, _, _ = _finish(mixed_keys(rng, g, kind, num_parts, table_keys), g, num_parts, bits, rng)
    return keys, (rng.random(keys.size) + 1e-3) * 1000., None
