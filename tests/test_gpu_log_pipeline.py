"""The counting sort and the reduce kernels behind the radiation-field log and the statistics log (skirt9_amd/csrc/pmc_log.inc:
rfHistKernel, rfScanKernel, rfScatterKernel, rfReduceKernel, statReduceKernel) on synthetic logs, on the MI355X.

Every radiation-field contribution of an octree run and every statistics contribution passes through these kernels.  The test aids of
include/pmc_tuning.h run them on logs that the host supplies (tests/log_checks.py builds them and holds the numpy references; tests/test_log_checks.py
checks both on the CPU).  The values of the logs are integer-valued doubles whose sums stay below 2^53: every sum is exact in any order, and every
comparison here is np.array_equal -- a lost, doubled or misplaced entry shows.  What lies beyond a chunk's fill is poison (key 0, value NaN).  One
pass per reduce kernel with non-integer values is compared with math.fsum under the worst-case bound of a sum in any order (log_checks.sum_bound).

Every edge -- partition counts around the lanes of the scan and of the scatter kernel, the limit of the LDS histograms, the short-run thresholds,
the reduce span, the chunk -- comes from Engine.log_geometry(): none is written down here.  The last tests send the photon loop's own logs through
partition counts above the scatter kernel's lanes."""
import numpy as np
import pytest

import log_checks as L
import oracle_lib as O
from conftest import ski
from scene_variants import with_field_grid, with_pixels, with_stored_field
from skirt9_amd.engine import Engine, set_tuning
from skirt9_amd.host import Simulation
from test_gpu_parity import _compare_frames

pytestmark = pytest.mark.gpu

# The accumulation tests bind a torch tensor as the radiation field table.  torch brings a HIP runtime of its own, and in a process in which the
# engine's runtime has opened the device first torch finds none; the other order works (see tests/test_gpu_temperature.py).  pytest imports every
# test module before it runs a test, so torch looks at the device here.  Without a GPU this is a quick no.
TORCH_PROBLEM = None
try:
    import torch
except ImportError as error:
    TORCH_PROBLEM = f"torch cannot be imported: {error}"
else:
    if torch.cuda.is_available():
        try:
            torch.cuda.init()
        except RuntimeError as error:
            TORCH_PROBLEM = f"torch sees a GPU and cannot open it: {error}"
    else:
        TORCH_PROBLEM = "torch sees no GPU"


class Context:
    """a scene, an engine on it, the engine's log geometry"""

    def __init__(self, path, num_packets=100, tuning=None):
        for name, value in (tuning or {}).items():
            set_tuning(name, value)
        self.sim = Simulation(path, num_packets=num_packets).setup()
        self.eng = Engine(self.sim.scene, 0)
        for name in tuning or {}:
            set_tuning(name, None)
        self.g = self.eng.log_geometry()
        self.name = None


def _context(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scenes")
    name = request.param
    if name == "cfg3rf":             # 6 bins: the table index of a key takes a division
        c = Context(ski("cfg3rf.ski"))
    elif name == "cfg3rf shuffled":  # the cell table in groups of 32 cells in scattered order: the device numbering has padding slots
        c = Context(ski("cfg3rf.ski"), tuning={"PMC_CELL_SHUFFLE": "5"})
    elif name == "cfg3rf 300 bins":  # more partitions than rfScatterKernel has lanes
        c = Context(with_field_grid(tmp, "cfg3rf", 300))
    elif name == "cfg2small":        # one wavelength: the table index of a key takes no division
        c = Context(with_stored_field(tmp, "cfg2small"))
    elif name == "cfg3small":
        c = Context(ski("cfg3small.ski"))
    elif name == "cfg3small 256 pixels":  # more partitions than rfScatterKernel has lanes
        c = Context(with_pixels(tmp, "cfg3small", "i0", 256))
    c.name = name
    yield c
    c.eng.close()


FIELD_CONTEXTS = ["cfg3rf", "cfg3rf shuffled", "cfg3rf 300 bins", "cfg2small"]
STAT_CONTEXTS = ["cfg3small", "cfg3small 256 pixels"]
field = pytest.fixture(scope="module", params=FIELD_CONTEXTS)(_context)
stats = pytest.fixture(scope="module", params=STAT_CONTEXTS)(_context)
small = pytest.fixture(scope="module", params=["cfg3rf"])(_context)

# ---- the counting sort alone


def _bits_of(g, stat):
    return g["stat_bucket_bits" if stat else "rf_bucket_bits"]


def _check_partition(c, stat, num_parts, log):
    keys, vals, fills = log
    bits = _bits_of(c.g, stat)
    got = c.eng.log_partition(stat, num_parts, keys, vals, fills)
    problem = L.partition_problem(keys, vals, fills, c.g["chunk"], bits, num_parts, *got)
    assert problem is None, (stat, num_parts, keys.size, problem)
    return got


PARTITION_COUNTS = {"1": lambda g: 1, "2": lambda g: 2, "T-1": lambda g: g["scan_threads"] - 1, "T": lambda g: g["scan_threads"],
                    "T+1": lambda g: g["scan_threads"] + 1, "B-1": lambda g: g["sort_block"] - 1, "B": lambda g: g["sort_block"],
                    "B+1": lambda g: g["sort_block"] + 1, "1000": lambda g: 1000, "MAX-1": lambda g: g["max_parts"] - 1, "MAX": lambda g: g["max_parts"]}


@pytest.mark.parametrize("count", list(PARTITION_COUNTS))
@pytest.mark.parametrize("stat", [0, 1])
def test_partition_counts(small, stat, count):
    """partition counts around the lanes of rfScanKernel (T) and of rfScatterKernel (B) -- beyond them a lane scans several partitions --
    and at the limit of the LDS histograms: three tiles, keys uniform over the partitions, 5 % pad keys, 5 % keys anywhere above"""
    g = small.g
    num_parts = PARTITION_COUNTS[count](g)
    assert g["scan_threads"] < g["sort_block"] < 1000 < g["max_parts"] - 1  # (the order the labels stand for)
    _, _, start = _check_partition(small, stat, num_parts, L.uniform_partition_log(g, _bits_of(g, stat), num_parts, 3, seed=num_parts + stat))
    assert 0.85 * 3 * g["chunk"] < start[-1] < 0.95 * 3 * g["chunk"]


@pytest.mark.parametrize("stat", [0, 1])
def test_partition_of_skewed_logs(small, stat):
    """all live entries in one partition -- the first, a middle one, the last -- over 1 tile, one reduce span of tiles, one more, and two spans
    and three tiles; pad keys only; one live entry; every 7th partition populated"""
    g = small.g
    bits, num_parts = _bits_of(g, stat), g["sort_block"] + 488
    span_tiles = g["reduce_span"] // g["chunk"]
    for tiles in (1, span_tiles, span_tiles + 1, 2 * span_tiles + 3):
        for part in (0, num_parts // 2, num_parts - 1):
            _, _, start = _check_partition(small, stat, num_parts, L.skewed_partition_log(g, bits, num_parts, tiles, [part], seed=tiles))
            assert start[part] == 0 and start[part + 1] == start[-1] == int(0.9 * tiles * g["chunk"])
    _, _, start = _check_partition(small, stat, num_parts, L.skewed_partition_log(g, bits, num_parts, 2, [], seed=1))
    assert start[-1] == 0
    _, _, start = _check_partition(small, stat, num_parts, L.skewed_partition_log(g, bits, num_parts, 2, [num_parts - 2], seed=2, live=1))
    assert start[-1] == 1 and start[num_parts - 2] == 0
    _, _, start = _check_partition(small, stat, num_parts, L.skewed_partition_log(g, bits, num_parts, 3, list(range(0, num_parts, 7)), seed=3))
    assert np.all((np.diff(start.astype(np.int64)) > 0) == (np.arange(num_parts) % 7 == 0))


@pytest.mark.parametrize("stat", [0, 1])
def test_partition_of_open_and_short_chunks(small, stat):
    """chunks filled 0, 1, 2, 3, 4, 5, B - 1, chunk - 1 and chunk entries in mixed order (launchPartition takes the fills for both
    instantiations); the rest of every chunk is poison: key 0 -- a live key of partition 0 -- and value NaN"""
    g = small.g
    bits = _bits_of(g, stat)
    for num_parts in (3, g["sort_block"] + 1):
        keys, vals, fills = L.filled_log(g, bits, num_parts, num_parts << bits, seed=num_parts)
        _, sorted_vals, start = _check_partition(small, stat, num_parts, (keys, vals, fills))
        assert not np.isnan(sorted_vals).any() and start[-1] < fills.sum()


# ---- the radiation-field reduce


def _field_numbers(c):
    g = c.g
    return g["rf_bucket_bits"], g["rf_parts"], g["rf_keys"], g["rf_num_lambda"], c.eng.radiation_field_size


def _flushed_field(c, log):
    c.eng.clear_radiation_field()
    c.eng.rf_log_flush(log[0], log[1])
    return c.eng.download_radiation_field()


def test_cell_numbering(field):
    """the device numbering the keys of the radiation-field log count cells in: its non-negative entries are a permutation of the cells.  The
    default numbering has no padding slot; the shuffled cell table (tuning switch PMC_CELL_SHUFFLE = 5: groups of 32 cells, 17 592 cells) has"""
    g, ext = field.g, field.eng.cell_numbering()
    assert g["rf_logged"] == 1 and ext.size == g["cell_slots"] and g["rf_keys"] == g["cell_slots"] * g["rf_num_lambda"]
    assert g["rf_parts"] == -(-g["rf_keys"] >> g["rf_bucket_bits"]) and field.eng.radiation_field_size == field.eng.num_cells * g["rf_num_lambda"]
    assert np.array_equal(np.sort(ext[ext >= 0]), np.arange(field.eng.num_cells))
    assert (ext < 0).sum() == g["cell_slots"] - field.eng.num_cells
    if field.name == "cfg3rf shuffled":
        assert (ext < 0).any() and not np.array_equal(ext[ext >= 0], np.arange(field.eng.num_cells))
    if field.name == "cfg3rf 300 bins":
        assert g["rf_parts"] > g["sort_block"]


@pytest.mark.parametrize("family", ["coverage", "threshold runs", "span edges", "mixed"])
def test_field_reduce(field, family):
    """coverage: every key of [0, rf_keys) once -- every mapping, every padding slot -- and every key up to the end of the last partition, which
    must vanish.  threshold runs: partitions with S - 1, S and S + 1 entries (S: below it a run is added entry by entry, from it on through LDS),
    all on one key and dealt over the partition's keys.  span edges: three reduce spans on ONE key (three workgroups, same-address LDS atomics),
    live totals of span - 1, span, span + 1, a span that begins inside a streak of empty partitions (contexts with enough partitions).  mixed:
    long and short runs side by side.  Bit for bit against np.add.at."""
    bits, parts, rf_keys, nl, size = _field_numbers(field)
    ext = field.eng.cell_numbering()
    seen = 0
    for name, log in L.reduce_logs(field.g, "rf", parts, rf_keys, families=(family,)):
        want = L.rf_reduce(log[0], log[1], ext, nl, rf_keys, size, parts, bits)
        got = _flushed_field(field, log)
        assert np.array_equal(got, want), (name, int((got != want).sum()), float(got.sum()), float(want.sum()))
        assert want.max() < L.EXACT
        if name == "coverage":
            assert np.count_nonzero(want) == size  # every entry of the table has been reached
        seen += 1
    assert seen >= 1


def test_field_reduce_of_non_integer_values(field):
    """random positive non-integer values against math.fsum per table entry; bound: (n_k - 1) 2^-53 sum|v| with n_k entries on the key, the worst
    case of a sum of n_k terms in any order (derived in tests/log_checks.py)"""
    bits, parts, rf_keys, nl, size = _field_numbers(field)
    keys, vals, _ = L.non_integer_log(field.g, "rf", parts, rf_keys)
    index = np.where(L.live_mask(keys, None, field.g["chunk"], bits, parts), L.rf_table_index(keys, field.eng.cell_numbering(), nl, rf_keys), -1)
    want, count, magnitude = L.fsum_by_key(index, vals, size)
    got = _flushed_field(field, (keys, vals))
    excess = np.abs(got - want) - L.sum_bound(count, magnitude)
    assert count.max() >= field.g["rf_short_run"] and np.array_equal(got != 0, count > 0)
    assert excess.max() <= 0., (int((excess > 0).sum()), float(excess.max()))


def test_field_accumulates(field):
    """the same log flushed twice into a bound table that holds 1.0 everywhere: 1 + 2 x the reference, bit for bit"""
    assert TORCH_PROBLEM is None, f"the bound table of this test is a torch tensor: {TORCH_PROBLEM}"
    eng = Engine(field.sim.scene, 0)  # (a context of its own, in the default numbering)
    g = eng.log_geometry()
    bits, parts, rf_keys, nl, size = g["rf_bucket_bits"], g["rf_parts"], g["rf_keys"], g["rf_num_lambda"], eng.radiation_field_size
    ext = eng.cell_numbering()
    table = torch.ones(size, dtype=torch.float64, device="cuda:0")
    eng.bind_radiation_field(table.data_ptr(), table.numel())
    (name, log), = L.reduce_logs(g, "rf", parts, rf_keys, families=("mixed",))
    eng.rf_log_flush(log[0], log[1])
    eng.rf_log_flush(log[0], log[1])
    got = eng.download_radiation_field()
    eng.close()
    want = 1. + 2. * L.rf_reduce(log[0], log[1], ext, nl, rf_keys, size, parts, bits)
    assert np.array_equal(got, want) and np.array_equal(table.cpu().numpy(), want)


def test_field_short_run_threshold_is_where_the_geometry_says(small):
    """With integer values both branches of rfReduceKernel give the same sums, so the tests above cannot tell on which side of rf_short_run a run
    went.  A table that holds 2^53 can: a run of n entries of 1.0 on one key that is added entry by entry leaves 2^53 (2^53 + 1 rounds to even,
    n times, in any order), a run that is summed in LDS first adds n at once.  rf_short_run - 1 entries: entry by entry; rf_short_run and
    rf_short_run + 1: through LDS.  (The statistics accumulator starts every flush at zero: there both branches add the same values to zero in an
    order of their own, and no result can tell them apart.)"""
    assert TORCH_PROBLEM is None, f"the bound table of this test is a torch tensor: {TORCH_PROBLEM}"
    eng = Engine(small.sim.scene, 0)
    g = eng.log_geometry()
    bits, parts, rf_keys, nl, size = g["rf_bucket_bits"], g["rf_parts"], g["rf_keys"], g["rf_num_lambda"], eng.radiation_field_size
    short, chunk, big = g["rf_short_run"], g["chunk"], 1 << 53
    table = torch.full((size,), float(big), dtype=torch.float64, device="cuda:0")
    eng.bind_radiation_field(table.data_ptr(), table.numel())
    want = np.full(size, float(big))
    for part, entries in ((0, short - 1), (parts // 2, short), (parts - 1, short + 1)):
        key = part << bits
        keys = np.full(-(-entries // chunk) * chunk, parts << bits, dtype=np.uint32)  # (filled up with pad keys)
        keys[:entries] = key
        eng.rf_log_flush(keys, np.ones(keys.size))
        at = L.rf_table_index([key], eng.cell_numbering(), nl, rf_keys)[0]
        assert at >= 0
        want[at] = float(big) if entries < short else float(big + entries)  # (int -> float rounds to even as the addition does)
    got = eng.download_radiation_field()
    eng.close()
    assert np.array_equal(got, want), [(int(i), got[i] - big, want[i] - big) for i in np.flatnonzero(got != want)[:5]]


# ---- the statistics reduce


def test_statistics_reduce(stats):
    """the families of test_field_reduce with the statistics threshold and records (count and the sums of w, w^2, w^3, w^4 per record: all five
    bit for bit), keys between the last record and the end of the last partition, and a log with open and short chunks whose rest is poison"""
    g = stats.g
    bits, parts, records = g["stat_bucket_bits"], g["stat_parts"], g["stat_records"]
    assert g["stat_logged"] == 1 and parts == -(-records >> bits)
    if stats.name == "cfg3small 256 pixels":
        assert parts > g["sort_block"]
    seen = set()
    for name, (keys, vals, fills) in L.reduce_logs(g, "stat", parts, records):
        want = L.stat_reduce(keys, vals, records, parts, bits, fills, g["chunk"])
        got = stats.eng.stat_log_flush(keys, vals, fills)
        assert got.shape == want.shape and not np.isnan(got).any(), name
        for power in range(5):
            assert np.array_equal(got[:, power], want[:, power]), (name, power, int((got[:, power] != want[:, power]).sum()))
        assert want.max() <= float(1 << 52)
        seen.add(name)
    assert {"coverage", "mixed", "open and short chunks", "three spans on one key"} <= seen
    # the flush leaves the accumulator empty: a log of pad keys adds nothing to it
    keys, vals, _ = L.skewed_partition_log(g, bits, parts, 1, [], seed=1)
    assert not stats.eng.stat_log_flush(keys, vals).any()


def test_statistics_reduce_of_non_integer_values(stats):
    """random positive non-integer weights against math.fsum per record and power; bound: (n_k - 1 + k) 2^-53 sum w^k (log_checks.sum_bound)"""
    g = stats.g
    bits, parts, records = g["stat_bucket_bits"], g["stat_parts"], g["stat_records"]
    keys, vals, _ = L.non_integer_log(g, "stat", parts, records)
    index = np.where(L.live_mask(keys, None, g["chunk"], bits, parts) & (keys < records), keys.astype(np.int64), -1)
    got = stats.eng.stat_log_flush(keys, vals)
    power = np.ones_like(vals)
    for k in range(5):
        want, count, magnitude = L.fsum_by_key(index, power, records)
        if k == 0:
            assert np.array_equal(got[:, 0], count.astype(np.float64)) and count.max() >= g["stat_short_run"]
        else:
            excess = np.abs(got[:, k] - want) - L.sum_bound(count, magnitude, power=k)
            assert excess.max() <= 0., (k, int((excess > 0).sum()), float(excess.max()))
        power = power * vals  # ((w w) w) w


# ---- argument errors


def test_refusals_leave_the_context_usable(small):
    """every aid refuses what could make a kernel read or write out of bounds, with PMC_ERR_INVALID and before anything is launched; the context
    then runs a segment like a fresh one"""
    g, eng = small.g, Engine(small.sim.scene, 0)
    chunk, bits = g["chunk"], g["rf_bucket_bits"]
    keys, vals, _ = L.uniform_partition_log(g, bits, 4, 2, seed=1)
    fills = np.array([chunk, 7], dtype=np.uint32)
    assert g["rf_logged"] == 1 and g["stat_logged"] == 1

    def refused(call, *args, **kwargs):
        with pytest.raises(RuntimeError, match="pmc error -1:"):
            call(*args, **kwargs)

    for aid in (lambda k, v: eng.log_partition(0, 4, k, v), lambda k, v: eng.log_partition(1, 4, k, v), eng.rf_log_flush, eng.stat_log_flush):
        refused(aid, keys[:chunk - 1], vals[:chunk - 1])   # no multiple of the chunk
        refused(aid, keys[:chunk + 4], vals[:chunk + 4])
        refused(aid, keys[:0], vals[:0])                   # no entry
        refused(aid, None, vals)                           # null arrays
        refused(aid, keys, None)
    big = g["max_entries"] + chunk                         # more entries than the aids take
    refused(eng.log_partition, 0, 4, np.zeros(big, dtype=np.uint32), np.zeros(big))
    refused(eng.rf_log_flush, np.zeros(big, dtype=np.uint32), np.zeros(big))
    refused(eng.stat_log_flush, np.zeros(big, dtype=np.uint32), np.zeros(big))
    for num_parts in (0, -1, g["max_parts"] + 1, 10 * g["max_parts"]):
        refused(eng.log_partition, 0, num_parts, keys, vals)
        refused(eng.log_partition, 1, num_parts, keys, vals)
    refused(eng.log_partition, 2, 4, keys, vals)           # no such instantiation
    too_full = np.array([chunk, chunk + 1], dtype=np.uint32)
    refused(eng.log_partition, 0, 4, keys, vals, too_full)
    refused(eng.log_partition, 1, 4, keys, vals, too_full)
    refused(eng.stat_log_flush, keys, vals, too_full)
    # a context without a logged field or without logged statistics: the switches that send the sums through atomics, a Cartesian grid (which
    # has no device numbering either), a scene that stores no field
    set_tuning("PMC_RF_ATOMICS", "1")
    assert eng.log_geometry()["rf_logged"] == 0
    refused(eng.rf_log_flush, keys, vals)
    set_tuning("PMC_RF_ATOMICS", None)
    set_tuning("PMC_STAT_ATOMICS", "1")
    assert eng.log_geometry()["stat_logged"] == 0
    refused(eng.stat_log_flush, keys, vals)
    set_tuning("PMC_STAT_ATOMICS", None)
    for name in ("cfg1rf.ski", "cfg3small.ski"):
        sim = Simulation(ski(name), num_packets=100).setup()  # (the scene lives as long as this object)
        other = Engine(sim.scene, 0)
        assert other.log_geometry()["rf_logged"] == 0
        refused(other.rf_log_flush, keys, vals)
        if name == "cfg1rf.ski":
            refused(other.cell_numbering)
        other.close()
    # what is accepted still works, and the context runs a segment like a fresh one
    start = eng.log_partition(0, 4, keys, vals, fills)[2]
    assert np.array_equal(start, L.partition_starts(keys, fills, chunk, bits, 4))
    eng.rf_log_flush(keys, vals)
    eng.stat_log_flush(keys, vals, fills)
    eng.clear_radiation_field()
    fresh = Engine(small.sim.scene, 0)
    n = 3000
    for e in (eng, fresh):
        e.run_primary(0, n, 7)
    a, b = eng.counters(), fresh.counters()
    assert a == b and a["histories"] == n
    fa, fb = eng.download(), fresh.download()
    assert np.allclose(fa, fb, rtol=1e-9, atol=1e-12 * np.abs(fb).max())
    ra, rb = eng.download_radiation_field(), fresh.download_radiation_field()
    assert np.allclose(ra, rb, rtol=1e-9, atol=1e-15 * rb.max()) and rb.sum() > 0
    eng.close()
    fresh.close()


# ---- through the photon loop: partition counts above the scatter kernel's lanes met by logs that the walk and launch kernels write


def test_photon_loop_field_on_300_bins(tmp_path):
    """cfg3rf with its field on 300 bins (645 partitions), 20 000 histories: the logged table against the oracle on the same Philox histories at
    the tolerances of test_radiation_field_matches_oracle (totals 1e-9, the same non-zero entries, elements 1e-6 relative + 1e-13 of the
    maximum), and against the run that adds every contribution atomically at those of the full-size test (totals 1e-11, elements 1e-9 + 1e-15
    of the maximum: the two differ in summation order only)"""
    n = 20000
    sim = Simulation(with_field_grid(tmp_path, "cfg3rf", 300), num_packets=n).setup()
    eng = Engine(sim.scene, 0)
    g = eng.log_geometry()
    assert g["rf_logged"] == 1 and g["rf_parts"] > g["sort_block"]  # (not through the atomic fallback)
    eng.run_primary(0, n, 5)
    logged = eng.download_radiation_field()
    eng.close()
    _, ref, _ = O.run_primary_rf(sim, 0, n, O.RNG_PHILOX, seed=5)
    assert abs(logged.sum() - ref.sum()) <= 1e-9 * ref.sum()
    assert np.array_equal(logged > 0, ref > 0)
    assert (np.abs(logged - ref) > 1e-6 * np.abs(ref) + 1e-13 * ref.max()).sum() == 0
    set_tuning("PMC_RF_ATOMICS", "1")
    eng = Engine(sim.scene, 0)
    assert eng.log_geometry()["rf_logged"] == 0
    eng.run_primary(0, n, 5)
    atomics = eng.download_radiation_field()
    eng.close()
    assert abs(logged.sum() - atomics.sum()) <= 1e-11 * atomics.sum()
    assert np.array_equal(logged > 0, atomics > 0)
    assert (np.abs(logged - atomics) > 1e-9 * np.abs(atomics) + 1e-15 * atomics.max()).sum() == 0


def test_photon_loop_statistics_on_256_pixels(tmp_path):
    """cfg3small with instrument i0 at 256 x 256 pixels (640 partitions for i0 alone), 40 000 histories in two segments: the statistics from the
    log, from a log of one chunk per group and from the atomic path alone, each against the oracle (test_statistics_log_matches_atomics_and_oracle)"""
    n = 40000
    sim = Simulation(with_pixels(tmp_path, "cfg3small", "i0", 256), num_packets=n).setup()
    ref, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=11)
    for switches in ({}, {"PMC_STAT_LOG_ENTRIES": "4096"}, {"PMC_STAT_ATOMICS": "1"}):
        for k, v in switches.items():
            set_tuning(k, v)
        eng = Engine(sim.scene, 0)
        g = eng.log_geometry()
        assert g["stat_logged"] == (0 if "PMC_STAT_ATOMICS" in switches else 1) and g["stat_parts"] > g["sort_block"]
        half = n // 2
        eng.run_primary(0, half, 11)
        eng.run_primary(half, n - half, 11)
        gpu = eng.download()
        assert eng.counters()["stat_overflows"] == 0
        _compare_frames(sim, gpu, ref, n)
        for k in switches:
            set_tuning(k, None)
        eng.close()
