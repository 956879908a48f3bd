"""The production walk kernels -- walkPropKernel, walkPeelKernel, walkPeelKernel2, walkKernel<Cart | Voro | Bin>, voroPeelKernel, voroPropKernel --
on walks that the HOST supplies (Engine.walk_cycle: one cycle start and one generation's walks of slot group 0, through pmc_run_primary's own
plan and enqueue functions), against tests/walk_checks.py: per slot ptau, sint, nint, mint, taupath and tausample bit for bit, the walk counters
exactly.  tests/test_walk_checks.py holds that restatement to the oracle's own path code, bit for bit, on the same scenes and rays.

What is NOT exact, and why: on the exponential branch of the sampled depth (u1 >= xi) the device's exp and log decide tausample, which is held to
an envelope measured against mpmath here; everything after it is exact again, given the device's tausample.  The re-walk counter of a propagation
kernel that keeps pass-1 checkpoints (Bench.may_resume: the plain forced flavour of walkPropKernel and voroPropKernel) depends on where the wave's
checkpoint tick fell: there it is bounded by the paths' count, everywhere else it equals it.  The
radiation field of the pass-1 walks holds the device's exp and, per cell, atomic additions in any order: bounded per entry (walk_checks.field_table)."""
import copy
import math

import numpy as np
import pytest

import walk_checks as W
from skirt9_amd.engine import set_tuning

pytestmark = pytest.mark.gpu

POOL = 4096          # slots of the engines' pools: one group of 4096
BIG = 256 * 12 + 29  # more slots than a workgroup's waves take from the cursor in one round (PMC_TASK_CHUNK x the twelve waves of the octree
                     # kernels; the generic kernel's workgroups have four)
UNSET = -1.          # include/pmc_tuning.h PMC_WALK_CYCLE_UNSET

# scene -> the committed rays it is probed with (as tests/test_walk_checks.py)
RAYS = {"cfg1": "cfg1", "cfg2small": "cfg2small", "cfg2deeper": "cfg2deeper", "cfg2bin": "cfg2bin", "cfg5small": "cfg5small", "cfg1nf": "cfg1",
        "cfg1nfea": "cfg1", "cfg2ea": "cfg2small", "cfg1mmnf": "cfg1", "cfg2mm": "cfg2small", "cfg2mmea": "cfg2small", "cfg3small": "cfg2small",
        "cfg3twelve": "cfg2small", "cfg1@60": "cfg1", "cfg2small@60": "cfg2small", "cfg2bin@60": "cfg2bin", "cfg5small@60": "cfg5small"}

_benches = {}
_open = []  # the benches whose engine is open, least recently used first (the library allows six live contexts per process)


class Bench:
    """a scene, its engine, and the deck of slots it is probed with (each with what the restatement expects of it)"""

    def __init__(self, name, tmp_path, poison=False, created_under=()):
        """created_under: the switches that are set while the engine is created (those that pmc_create samples), besides the poison"""
        self.name, self.poison, self.created_under, self._eng = name, poison, tuple(created_under), None
        self.sc = W.load_scene(name, tmp_path, num_packets=20000)
        try:
            self.ext = self.eng.cell_numbering()   # tree grids: device cell -> the caller's
        except RuntimeError:
            self.ext = np.arange(self.sc.num_cells, dtype=np.int32)
        self.dev = np.full(self.sc.num_cells, -1, dtype=np.int32)
        self.dev[self.ext[self.ext >= 0]] = np.nonzero(self.ext >= 0)[0]
        self._paths = {}
        self.deck = self._deck()

    @property
    def eng(self):
        """the scene's engine: opened when it is needed, closed when three others have been used since"""
        from skirt9_amd.engine import Engine
        if self._eng is None:
            if self.poison:
                set_tuning("PMC_POISON_ALLOCATIONS")   # (sampled at every allocation: stays set for the rest of the test)
            for switch in self.created_under:
                set_tuning(switch)
            try:
                self._eng = Engine(self.sc.sim.scene, 0)
            finally:
                for switch in self.created_under:
                    set_tuning(switch, None)
            self._eng.set_num_slots(POOL)
        if self in _open:
            _open.remove(self)
        _open.append(self)
        while len(_open) > 3:
            old = _open.pop(0)
            old._eng.close()
            old._eng = None
        return self._eng

    def path(self, r, k):
        key = (r.tobytes(), k.tobytes())
        if key not in self._paths:
            self._paths[key] = self.sc.path(r, k)
        return self._paths[key]

    def slot(self, r, k, mask, weights, u1=0., u2=0.5, depth=1., hint=-1, sext=None, taumax=None):
        """a slot and what the walks must leave in it; None when a path of it is too long for the oracle's buffer.  sext: the extinction cross
        section that travels with the slot's packet instead of the dust mix's (a scene with more than one wavelength and one medium component,
        no explicit absorption); taumax: the stop values of the peel-off walks where they are not the host's peelTaumax of the weights"""
        sc = self.sc
        if sext is not None:
            assert not sc.mm and not sc.ea
            sc = copy.copy(sc)
            sc.sext = [sext]
        s = dict(r=np.array(r, dtype=np.float64), k=np.array(k, dtype=np.float64), mask=0, ppW=np.zeros(sc.num_instruments), u1=u1, u2=u2,
                 depth=depth, hint=hint, ptau=np.full(sc.num_instruments, UNSET), visits=0, paths=1, sext=sc.sext[0])
        for q, (inst, w) in enumerate(zip(mask, weights)):
            path = self.path(s["r"], sc.kobs[inst])
            if path is None:
                return None
            s["mask"] |= 1 << (8 + inst)
            s["ppW"][inst] = w
            s["ptau"][inst], visits = W.peel(sc, path, taumax[q] if taumax else W.peel_taumax(w, sc.wavelength))
            s["visits"] += visits
            s["paths"] += 1
        path = self.path(s["r"], s["k"])
        if path is None:
            return None
        s["prop"] = W.forced(sc, path, u1, u2) if sc.forced else W.non_forced(sc, path, depth)
        s["visits"] += s["prop"]["visits"]
        s["rewalks"] = s["prop"].get("rewalks", 0)
        s["paths"] += 1 if s["prop"].get("taupath") is not None else 0
        return s

    def stop_weight(self, r, inst):
        path = self.path(r, self.sc.kobs[inst])
        if path is None or len(path[0]) == 0:
            return None
        got = W.peel_weight_between(self.sc, W.partial_sums(self.sc, path, apart=False), lambda w: W.peel_taumax(w, self.sc.wavelength))
        return got[0] if got else None

    def _deck(self):
        sc, L = self.sc, self.sc.leaders
        rays = W.golden_rays(RAYS[self.name])
        masks = [[], L[:1], L[::2], L]  # none, one, some, all observers: mixed within every wave
        deck = []

        def weights(r, mask, turn):
            out = []
            for inst in mask:
                choice = [sc.wavelength, 0., -1., self.stop_weight(r, inst)][(turn + inst) % 4]  # taumax = 745 exactly; no luminosity; a stop inside
                out.append(sc.wavelength if choice is None else choice)
            return out
        for j, (r, k) in enumerate(rays):
            path = self.path(r, k)
            if path is None:
                continue
            if sc.forced:
                draws = [dict(u1=0., u2=u2) for u2 in W.FORCED_U2]
            else:
                sums = W.partial_sums(sc, path)
                distinct = sorted(set(t for t in sums if t > 0.))
                picked = distinct[:2] + distinct[len(distinct) // 2:len(distinct) // 2 + 1] + distinct[-2:]
                draws = [dict(depth=d) for d in W.non_forced_depths(sorted(set(picked)) or [0.])]
            for q, draw in enumerate(draws):
                mask = masks[(j + q) % 4]
                deck.append(self.slot(r, k, mask, weights(r, mask, j + q), **draw))
        for inst in L:
            for j, r in enumerate(W.peel_positions(sc, rays, inst)[len(rays):]):
                mask = [inst] if j % 3 else L
                deck.append(self.slot(r, rays[j % len(rays)][1], mask, weights(r, mask, j + 3)))
        return [s for s in deck if s is not None]

    def run(self, slots, **form):
        sc, n = self.sc, len(slots)
        args = dict(r=[s["r"] for s in slots], k=[s["k"] for s in slots], mask=[s["mask"] for s in slots],
                    ppW=np.array([s["ppW"] for s in slots]).T, hint=[s["hint"] for s in slots],
                    wavelength=np.full(n, sc.wavelength), dust_ext=[s["sext"] for s in slots], dust_sca=np.full(n, sc.ssca[0]), dust_abs=np.full(n, sc.sabs[0]),
                    dust_idx=np.repeat(np.array(sc.index, dtype=np.int32), n))
        if sc.forced:
            args.update(u1=[s["u1"] for s in slots], u2=[s["u2"] for s in slots])
        else:
            args.update(depth=[s["depth"] for s in slots])
        args.update(form)
        return self.eng.walk_cycle(**args)

    def check(self, slots, res, switches=(), exponential=False):
        """every per-slot result bit for bit, the counters exactly; switches: the tuning switches the call ran under"""
        sc = self.sc
        assert res["internal_errors"] == 0
        want_ptau = np.array([s["ptau"] for s in slots]).T
        bad = np.nonzero(W.bits(res["ptau"]) != W.bits(want_ptau))
        assert bad[0].size == 0, (self.name, "ptau", list(zip(*bad))[:5], res["ptau"][bad][:5], want_ptau[bad][:5])
        for i, s in enumerate(slots):
            p = s["prop"]
            where = (self.name, i, s["r"], s["k"], s["u1"], s["u2"], s["depth"])
            if p["mint"] < 0:
                assert res["mint"][i] == -1, where
                continue
            if exponential:  # (what follows the sampled depth, for the DEVICE's depth)
                p = W.forced(sc, self.path(s["r"], s["k"]), s["u1"], s["u2"], tausample=res["tausample"][i])
            assert res["mint"][i] >= 0 and self.ext[res["mint"][i]] == p["mint"], where + (res["mint"][i], p["mint"])
            if sc.forced:
                assert W.bits(res["taupath"][i:i + 1])[0] == W.bits([p["taupath"]])[0], where
                assert W.bits(res["tausample"][i:i + 1])[0] == W.bits([p["tausample"]])[0], where
            for field in ("sint", "nint"):
                assert W.bits(res[field][i:i + 1])[0] == W.bits([p[field]])[0], where + (field, res[field][i], p[field])
        if not exponential:
            assert res["visits"] == sum(s["visits"] for s in slots), self.name
            assert res["paths"] == sum(s["paths"] for s in slots), self.name
            rewalks = sum(s["rewalks"] for s in slots)
            if rewalks == 0 or not self.may_resume(switches):
                assert res["rewalks"] == rewalks, (self.name, switches, res["rewalks"], rewalks)
            else:
                assert 0 < res["rewalks"] <= rewalks, (self.name, switches, res["rewalks"], rewalks)

    def may_resume(self, switches=()):
        """may pass 2 of a walk resume from a pass-1 checkpoint instead of the path's start?  Then the re-walk counter depends on where the
        wave's checkpoint tick fell and is only bounded by the path's count; everywhere else it is the path's count exactly.  Checkpoints
        are kept by walkPropKernel and voroPropKernel in their plain forced flavour only (no explicit absorption, one medium component), not
        under PMC_PROP_NO_CHECKPOINTS (the octree samples it at the run, a Voronoi context when it is created); the generic walkKernel --
        Cartesian, binary tree, and Voronoi without its propagation kernel or without the sort that feeds it -- keeps none"""
        sc = self.sc
        if not sc.forced or sc.ea or sc.mm or sc.grid_kind not in (W.GRID_OCTREE, W.GRID_VORONOI):
            return False
        if sc.grid_kind == W.GRID_OCTREE:
            return "PMC_PROP_NO_CHECKPOINTS" not in switches
        return "PMC_PROP_NO_CHECKPOINTS" not in self.created_under and not {"PMC_VORO_NO_PROP_KERNEL", "PMC_NO_PEEL_SORT"} & set(switches)


@pytest.fixture(scope="module", autouse=True)
def _engines_closed_at_the_end():
    """no context of this module stays open for the modules after it"""
    yield
    while _open:
        b = _open.pop()
        b._eng.close()
        b._eng = None
    _benches.clear()


@pytest.fixture
def bench(tmp_path_factory):
    def load(name, poison=False, created_under=()):
        key = (name, poison, tuple(created_under))
        if key not in _benches:
            _benches[key] = Bench(name, tmp_path_factory.mktemp("ski"), poison, created_under)
        return _benches[key]
    return load


ALL = ["cfg1", "cfg2small", "cfg2deeper", "cfg2bin", "cfg5small", "cfg1nf", "cfg1nfea", "cfg2ea", "cfg1mmnf", "cfg2mm", "cfg2mmea", "cfg3small",
       "cfg3twelve", "cfg1@60", "cfg2small@60", "cfg2bin@60", "cfg5small@60"]


@pytest.mark.parametrize("name", ALL)
def test_deck_bit_for_bit(name, bench):
    """every slot of the scene's deck in one call, as the group's slot range: propagation walks of every committed ray with every u2 of FORCED_U2
    (forced) or the depths around the path's partial sums (not forced); peel-off walks from ray starts, grid corners, edges and faces, from
    outside the grid, past it and behind it, with masks of none, one, some and all observers mixed in every wave and weights that give
    taumax = 745, no luminosity, and (the optically thick variants) a stop inside the path"""
    b = bench(name)
    assert len(b.deck) >= 300 and len(b.deck) <= POOL
    kinds = [s["prop"]["mint"] >= 0 for s in b.deck]
    assert any(kinds) and not all(kinds)                                       # walks that interact and walks that end the history
    assert any(s["mask"] and s["prop"].get("visits", 0) == 0 for s in b.deck)  # peel-off walks without a propagation walk
    finite = [t for s in b.deck for t in s["ptau"] if t != UNSET]
    assert any(t == 0. for t in finite) and any(0. < t < math.inf for t in finite) and any(t == math.inf for t in finite)
    if "@" in name:
        stops = sum(1 for s in b.deck for i in b.sc.leaders if s["ptau"][i] == math.inf and s["ppW"][i] > 0.)
        assert stops >= 10, stops
    b.check(b.deck, b.run(b.deck))


@pytest.mark.parametrize("name", ["cfg1", "cfg2small", "cfg2deeper", "cfg2bin", "cfg5small", "cfg1nf", "cfg3small"])
def test_slot_counts(name, bench):
    """1, 63, 64, 65 slots and more than a workgroup takes from the cursor in a round: all on the same ray, and every slot another one of
    the deck in a permuted order"""
    b = bench(name)
    rng = np.random.default_rng(7)
    busy = next(s for s in b.deck if s["mask"] and s["prop"]["mint"] >= 0)
    for n in (1, 63, 64, 65, BIG):
        same = [busy] * n
        b.check(same, b.run(same))
        mixed = [b.deck[i % len(b.deck)] for i in rng.permutation(max(n, len(b.deck)))[:n]]
        b.check(mixed, b.run(mixed))


FORMS = [("PMC_SERIAL_WALKS",), ("PMC_NO_XCD_AFFINITY",), ("PMC_NO_LIVE_LISTS",), ("PMC_NO_PEEL_SORT",), ("PMC_PROP_NO_CHECKPOINTS",),
         ("PMC_VORO_NO_PEEL_KERNEL",), ("PMC_VORO_NO_PROP_KERNEL",), ("PMC_VORO_NO_PEEL_KERNEL", "PMC_VORO_NO_PROP_KERNEL")]


@pytest.mark.parametrize("name", ["cfg1", "cfg2bin", "cfg2small", "cfg2deeper", "cfg5small", "cfg3small", "cfg3twelve", "cfg2mm"])
def test_forms_give_the_same_bits(name, bench):
    """the deck under every switch that selects another form of the walk kernels or of their task claiming: the same bits per slot as the plain
    form, and the restatement's.  (cfg3small sorts the peel-off records of its three observers, cfg3twelve has more observers than the sort takes;
    without the sort the generic kernel of cfg1, cfg2bin -- three observers -- and cfg5small chains a slot's records in one lane.)"""
    b = bench(name)
    plain = b.run(b.deck)
    b.check(b.deck, plain)
    for form in FORMS:
        if any(s.startswith("PMC_VORO") for s in form) != (name == "cfg5small"):
            continue
        try:
            for switch in form:
                set_tuning(switch)
            res = b.run(b.deck)
        finally:
            for switch in form:
                set_tuning(switch, None)
        for field in ("ptau", "sint", "nint", "taupath", "tausample"):
            assert np.array_equal(W.bits(res[field]), W.bits(plain[field])), (name, form, field)
        assert np.array_equal(res["mint"], plain["mint"]), (name, form)
        b.check(b.deck, res, switches=form)


def test_voronoi_propagation_kernel_without_checkpoints(bench):
    """a Voronoi context created under PMC_PROP_NO_CHECKPOINTS: voroPropKernel walks pass 2 from the path's start, and its re-walk counter is
    the paths' count exactly (check); the per-slot bits are those of the context with checkpoints"""
    b = bench("cfg5small", created_under=("PMC_PROP_NO_CHECKPOINTS",))
    assert not b.may_resume() and bench("cfg5small").may_resume()
    res = b.run(b.deck)
    b.check(b.deck, res)
    plain = bench("cfg5small").run(b.deck)
    for field in ("ptau", "sint", "nint", "taupath", "tausample"):
        assert np.array_equal(W.bits(res[field]), W.bits(plain[field])), field
    assert np.array_equal(res["mint"], plain["mint"])
    assert plain["rewalks"] <= res["rewalks"]


@pytest.mark.parametrize("name", ["cfg2small", "cfg5small"])
def test_poisoned_allocations_give_the_same_bits(name, bench):
    """a context whose uninitialised device arrays hold 0xA5 bytes: nothing the walks read was left unwritten"""
    b = bench(name, poison=True)
    b.check(b.deck, b.run(b.deck))
    some = b.deck[:65]
    b.check(some, b.run(some))


@pytest.mark.parametrize("name", ["cfg2small", "cfg2deeper", "cfg3small", "cfg2ea"])
def test_live_list_form(name, bench):
    """the slots as the list of live slots of a sparse generation (octree), in ascending and in permuted order, for list lengths around a wave and
    beyond a workgroup's round: the bits of the slot-range form"""
    b = bench(name)
    assert b.eng.walk_cycle_limits()[1]
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, len(b.deck)):
        slots = b.deck[:n]
        b.check(slots, b.run(slots, live_list=True))
        b.check(slots, b.run(slots, live_list=True, order=rng.permutation(n)))
    set_tuning("PMC_NO_LIVE_LISTS")
    with pytest.raises(RuntimeError, match="keeps no lists"):
        b.run(b.deck[:4], live_list=True)


@pytest.mark.parametrize("name", ["cfg2small", "cfg2deeper", "cfg2bin", "cfg5small"])
def test_hints_do_not_change_the_results(name, bench):
    """mint as the hint for the first cell: none, the leaf of the position, the leaf of a neighbouring position (the second cell of the
    slot's path)"""
    b = bench(name)
    slots = []
    for s in b.deck[::3]:
        path = b.path(s["r"], s["k"])
        inside = [int(m) for m in path[0] if m >= 0]
        if len(path[0]) < 3 or path[0][0] < 0:
            continue
        slots.append(dict(s, hint=int(b.dev[inside[0]])))
        slots.append(dict(s, hint=int(b.dev[inside[1]])))
        slots.append(dict(s, hint=int(b.dev[inside[-1]])))
        slots.append(s)
    assert len(slots) >= 100
    b.check(slots, b.run(slots))


@pytest.mark.parametrize("name", ["cfg1", "cfg2small", "cfg5small", "cfg2ea", "cfg2mm"])
def test_exponential_branch(name, bench):
    """u1 >= xi: the device's tausample within 4 x the restatement's own error against mpmath on these inputs + 16 ulp (walk_checks.py
    exponential_budget); then sint, nint and mint bit for bit as the restatement gives them for the DEVICE's tausample"""
    import mpmath as mp
    b = bench(name)
    sc = b.sc
    slots = []
    for j, (r, k) in enumerate(W.golden_rays(RAYS[name])):
        # (u2 stays away from 1: there the computed depth can exceed tau_path by rounding, and the rejection round that follows continues
        # the slot's random stream, which is not restated here)
        for q, u2 in enumerate([2. ** -53, 1e-9, 0.03, 0.25, 0.5, 0.77, 0.999, 1. - 2. ** -20]):
            s = b.slot(r, k, [], [], u1=[0.5, 0.75, 1. - 2. ** -53][(j + q) % 3], u2=u2)
            if s is not None and s["prop"]["mint"] >= 0 and not s["prop"]["exact"]:
                assert s["prop"]["tausample"] < s["prop"]["taupath"] * (1. - 1e-9)
                slots.append(s)
    assert len(slots) >= 100
    exact, room, envelope = W.exponential_budget([(s["prop"]["taupath"], s["u2"]) for s in slots])
    print(f"{name}: exponential branch, {len(slots)} walks, envelope of the restatement for d >= 1/8: {max(v for e, v in envelope.items() if e >= -2):.2g}, "
          f"at 2^-8: {envelope.get(-7, 0.):.2g}, at 2^-30: {envelope.get(-29, 0.):.2g}, below 2^-53: {max([v for e, v in envelope.items() if e < -52] or [0.]):.2g}")
    res = b.run(slots)
    for i, s in enumerate(slots):
        assert abs(mp.mpf(float(res["tausample"][i])) - exact[i]) <= room[i], (name, i, s["u2"], s["prop"]["taupath"], res["tausample"][i], float(exact[i]))
        assert res["tausample"][i] <= s["prop"]["taupath"]
    b.check(slots, res, exponential=True)


@pytest.mark.parametrize("name", ["cfg1", "cfg2small", "cfg5small", "cfg1nf"])
def test_paths_without_optical_depth_end_the_history(name, bench):
    """rays that miss the grid, and rays through empty cells only: mint = -1, nothing else of the slot's results written"""
    b = bench(name)
    lo, hi = W.grid_box(b.sc.sim)
    size = float(np.max(hi - lo))
    slots = []
    for r, k in W.golden_rays(RAYS[name]):
        away = hi + size * np.array([1., 2., 3.])
        slots.append(b.slot(away, k if np.dot(k, away) > 0 else -k, [], []))
        path = b.path(r, k)
        if path is not None and len(path[0]) and not W.partial_sums(b.sc, path)[-1] > 0.:
            slots.append(b.slot(r, k, [], []))
    res = b.run(slots)
    b.check(slots, res)
    assert np.all(res["mint"] == -1) and np.all(res["taupath"] == UNSET) and res["rewalks"] == 0
    if b.sc.forced:
        assert np.all(res["tausample"] == UNSET)


def test_peel_stop_value_equal_to_the_path_depth(bench):
    """tau >= taumax stops a peel-off walk: a stop value EQUAL to the optical depth of the whole path gives inf, the next stop value above
    it the depth itself.  The scene has more than one wavelength, so the extinction cross section travels with the slot: it is stepped ulp by
    ulp until the path's depth is a double that a stop value can take (745 + a logarithm near -690: multiples of 2^-43), above 52 so that the
    weight is a normal double; the DEVICE's own peelTaumax (Engine.device_function) picks the weights, so that no bit of its log is assumed."""
    b = bench("cfg5small")
    sc, inst = b.sc, b.sc.leaders[0]
    rays = W.golden_rays(RAYS["cfg5small"])
    slots = []
    for r in W.peel_positions(sc, rays, inst):
        path = b.path(r, sc.kobs[inst])
        if path is None or len(path[0]) < 3 or not W.partial_sums(sc, path, apart=False)[-1] > 0.:
            continue
        sext = sc.sext[0] * 60. / W.partial_sums(sc, path, apart=False)[-1]
        for _ in range(400):
            sext = float(np.nextafter(sext, math.inf))
            thick = copy.copy(sc)
            thick.sext = [sext]
            t = W.partial_sums(thick, path, apart=False)[-1]
            if t > 52. and (t - 745.) + 745. == t and float(np.nextafter(t - 745., 0.)) + 745. > t:
                break
        else:
            continue
        # weights around lambda exp(t - 745), 12 ulp apart: the device's stop values of them step through t and its neighbours
        centre = sc.wavelength * math.exp(t - 745.)
        candidates = centre * (1. + 12 * 2. ** -52 * np.arange(-400, 401))
        stops = b.eng.device_function("peel_taumax", np.stack([candidates, np.full(candidates.size, sc.wavelength)], axis=1))[:, 0]
        at, above = np.nonzero(stops == t)[0], np.nonzero(stops > t)[0]
        if at.size == 0 or above.size == 0:
            continue
        for q in (at[at.size // 2], above[0]):
            slots.append(b.slot(r, rays[len(slots) % len(rays)][1], [inst], [float(candidates[q])], sext=sext, taumax=[float(stops[q])]))
            assert slots[-1]["ptau"][inst] == (math.inf if stops[q] == t else t)
        if len(slots) >= 24:
            break
    assert len(slots) >= 12, len(slots)
    b.check(slots, b.run(slots))


@pytest.mark.parametrize("base", ["cfg1", "cfg2small"])
def test_radiation_field_of_the_pass_1_walks(base, tmp_path):
    """the radiation-field flavour (walkKernel<Cart, RF>: atomic additions; walkPropKernel<RF>: the log, flushed by the aid as the next generation
    would): the table after one cycle of every committed ray, several times over with different luminosities, against L lnmean(e^-tau1, e^-tau0) ds
    summed per cell in 200-bit arithmetic.  Bound per entry (walk_checks.field_table): 4 x the restatement's measured error + (n - 1) u sum|v|"""
    from scene_variants import with_stored_field
    from skirt9_amd.engine import Engine
    from skirt9_amd.host import Simulation
    sc = W.Scene(Simulation(with_stored_field(tmp_path, base), num_packets=1000).setup())
    ell = sc.field_bin
    assert sc.rf and sc.forced and ell >= 0
    rays = [(r, k) for r, k in W.golden_rays(base) if sc.path(r, k) is not None]
    lums = [1., 0.37, 2.5e3, 1e-9, 3.]
    # (a slot carries the weight W = L lambda; the kernel forms the luminosity as W / lambda, and so does the reference here)
    weights = [lums[(i + j) % len(lums)] * sc.wavelength for j in range(5) for i in range(len(rays))]
    slots = [(r, k, w / sc.wavelength) for (r, k), w in zip(rays * 5, weights)]
    exact, room, envelope = W.field_table(sc, [(sc.path(r, k), lum) for r, k, lum in slots], sc.sim.radiation_field_size // sc.num_cells, ell)
    print(f"{base}: {len(slots)} pass-1 walks, {np.count_nonzero(exact)} cells, envelope of the restated contributions {envelope:.3g}")
    assert np.count_nonzero(exact) >= 300
    eng = Engine(sc.sim.scene, 0)
    eng.set_num_slots(POOL)
    eng.clear_radiation_field()
    n, bins = len(slots), sc.sim.radiation_field_size // sc.num_cells
    # (outside the field's grid: rfell = -1 for a fifth of the slots' twins, which must add nothing)
    res = eng.walk_cycle(r=[s[0] for s in slots] * 2, k=[s[1] for s in slots] * 2, mask=np.zeros(2 * n, dtype=np.int32), ppW=np.zeros((sc.num_instruments, 2 * n)),
                         u1=np.zeros(2 * n), u2=np.full(2 * n, 0.5), W=weights * 2, rfell=[ell] * n + [-1] * n,
                         wavelength=np.full(2 * n, sc.wavelength), dust_ext=np.full(2 * n, sc.sext[0]), dust_sca=np.full(2 * n, sc.ssca[0]))
    assert res["internal_errors"] == 0
    table = eng.download_radiation_field().reshape(sc.num_cells, bins)
    eng.close()
    assert np.count_nonzero(np.delete(table, ell, axis=1)) == 0
    bad = np.nonzero(np.abs(table[:, ell] - exact) > room)[0]
    assert bad.size == 0, (base, bad[:5], table[bad[:5], ell], exact[bad[:5]], room[bad[:5]])


def test_refusals(bench):
    """everything is checked before a launch"""
    b = bench("cfg2small")
    ok = b.deck[:8]

    def refused(match, slots=ok, **change):
        with pytest.raises(RuntimeError, match=match):
            b.run(slots, **change)
    bad = dict(ok[0], r=np.array([math.nan, 0., 0.]))
    refused("not finite", [bad] + ok)
    refused("unit vector", [dict(ok[0], k=np.array([0.6, 0.6, 0.6]))])
    refused("unit vector", [dict(ok[0], k=np.array([0., 0., 1. + 1e-11]))])
    refused("bits outside", mask=[1] * 8)
    refused("leads no observer", mask=[1 << 9] * 8)
    refused("hint", hint=[b.ext.size] * 8)
    refused("hint", hint=[-2] * 8)
    pad = np.nonzero(b.ext < 0)[0]
    if pad.size:
        refused("hint", hint=[int(pad[0])] * 8)
    refused(r"uniform outside", u2=[1.] * 8)
    refused("nscatt", nscatt=[0] * 8)
    refused("slot group 0 has", [ok[0]] * (POOL + 1))
    refused("permutation", live_list=True, order=[0] * 8)
    refused("at least one slot", [])
    with pytest.raises(ValueError, match="dust_idx"):  # (the wrapper refuses an array shorter than the library would read)
        b.run(ok, dust_idx=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="u2"):
        b.run(ok, u2=[0.5] * 7)
    b.check(ok, b.run(ok))


@pytest.mark.parametrize("name", ["cfg2small", "cfg5small", "cfg1nf"])
def test_a_real_run_afterwards(name, bench):
    """run_primary on a context that has run walk cycles: the counters and the integer-count rows of the statistics of a fresh context bit for
    bit, its frames to the parity tests' comparison"""
    from skirt9_amd.engine import Engine
    from test_gpu_parity import _compare_frames
    b = bench(name)
    b.check(b.deck, b.run(b.deck))
    n = 20000
    sim = b.sc.sim
    b.eng.reset_counters()
    b.eng.clear()
    b.eng.run_primary(0, n, 1)
    used, used_counters = b.eng.download(), b.eng.counters()
    fresh = Engine(sim.scene, 0)
    fresh.set_num_slots(POOL)
    fresh.run_primary(0, n, 1)
    ref, ref_counters = fresh.download(), fresh.counters()
    fresh.close()
    b.eng.clear()
    assert used_counters == ref_counters
    for inst in range(b.sc.num_instruments):
        lay = sim.layout(inst)
        # (the sum of w^0 is the first of an instrument's five statistics arrays: counts; an offset of -1: the instrument has none)
        for off, size in ((lay.wsed_offset, lay.num_lambda), (lay.wifu_offset, lay.npix * lay.num_lambda)):
            if off >= 0:
                assert np.array_equal(W.bits(used[off:off + size]), W.bits(ref[off:off + size])), (name, inst)
    _compare_frames(sim, used, ref, n)
