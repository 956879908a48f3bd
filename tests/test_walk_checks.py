"""tests/walk_checks.py -- the restatement of what a walk kernel leaves in a slot -- against the oracle's own path code (oracle_walk_result:
getExtinctionOpticalDepth, setExtinctionOpticalDepths + findInteractionPoint, the non-forced loop), bit for bit, on the scenes and rays
tests/test_gpu_walk_kernels.py sends to the device.  No GPU."""
import math

import numpy as np
import pytest

import walk_checks as W

# scene -> the committed rays it is probed with (a scene without rays of its own: those of the scene whose grid it shares)
SCENES = {"cfg1": "cfg1", "cfg2small": "cfg2small", "cfg2deeper": "cfg2deeper", "cfg2bin": "cfg2bin", "cfg5small": "cfg5small", "cfg1nf": "cfg1",
          "cfg1nfea": "cfg1", "cfg2ea": "cfg2small", "cfg1mmnf": "cfg1", "cfg2mm": "cfg2small", "cfg2mmea": "cfg2small", "cfg3small": "cfg2small",
          "cfg3twelve": "cfg2small",
          # (optically thick variants: the peel-off walks that stop inside their path)
          "cfg1@60": "cfg1", "cfg2small@60": "cfg2small", "cfg2bin@60": "cfg2bin", "cfg5small@60": "cfg5small"}
_scenes = {}


@pytest.fixture
def scene(tmp_path_factory):
    def load(name):
        if name not in _scenes:
            _scenes[name] = W.load_scene(name, tmp_path_factory.mktemp("ski"))
        return _scenes[name]
    return load


def same(a, b):
    return W.bits([a])[0] == W.bits([b])[0]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_peel_restatement_equals_the_oracle(name, scene):
    """ptau and the visit count of a peel-off walk towards every observer, from every start of peel_positions, for a weight that never stops
    the walk (taumax = 745), one without luminosity, and one that stops it between two partial sums"""
    sc = scene(name)
    rays = W.golden_rays(SCENES[name])
    hits = stops = 0
    for inst in sc.leaders:
        kobs = sc.kobs[inst]
        for r in W.peel_positions(sc, rays, inst):
            path = sc.path(r, kobs)
            if path is None:
                continue
            sums = W.partial_sums(sc, path, apart=False)
            weights = [sc.wavelength, 0., -1.]
            between = W.peel_weight_between(sc, sums, lambda w: W.peel_taumax(w, sc.wavelength))
            if between:
                weights.append(between[0])
            for w in weights:
                got, visits = W.peel(sc, path, W.peel_taumax(w, sc.wavelength))
                ref, _, ref_visits = sc.oracle(0, r, kobs, w)
                assert same(got, ref[0]), (name, inst, r, w, got, ref[0])
                # (a packet without luminosity: the oracle returns before it walks; the kernels start no walk for it either)
                assert visits == ref_visits, (name, inst, r, w)
            hits += len(path[0]) > 0
            if between:
                assert W.peel(sc, path, W.peel_taumax(between[0], sc.wavelength)) == (math.inf, between[1] + 1 - sum(1 for m in path[0][:between[1]] if m < 0))
                stops += 1
    assert hits >= 20 and (stops >= 10 or "@" not in name), (hits, stops)


@pytest.mark.parametrize("name", [n for n in sorted(SCENES) if n not in ("cfg1nf", "cfg1nfea", "cfg1mmnf")])
def test_forced_restatement_equals_the_oracle(name, scene):
    """tau_path, interaction cell, distance and (explicit absorption) absorption depth of a forced walk for every committed ray and every
    u2 of FORCED_U2 on the linear branch, and for depths of the exponential branch"""
    sc = scene(name)
    assert sc.forced and sc.xi > 0.
    checked = 0
    for r, k in W.golden_rays(SCENES[name]):
        path = sc.path(r, k)
        if path is None:
            continue
        for u1, u2 in [(0., u2) for u2 in W.FORCED_U2] + [(0.75, 0.3), (0.999, 1. - 2. ** -53), (0.5, 2. ** -53)]:
            got = W.forced(sc, path, u1, u2)
            value = got.get("tausample", 0.)
            ref, cell, visits = sc.oracle(1, r, k, value)
            assert got["visits"] == visits
            if got["taupath"] is None:
                assert not ref[0] > 0. and got["mint"] == -1
                continue
            assert same(got["taupath"], ref[0]), (name, r, k)
            assert got["mint"] == cell, (name, r, k, u1, u2)
            assert same(got["sint"], ref[1]), (name, r, k, u1, u2, got["sint"], ref[1])
            if sc.ea:
                assert same(got["nint"], ref[2]), (name, r, k, u1, u2)
            else:
                assert same(got["nint"], sc.dens[0][cell])
            assert got["exact"] == (u1 < sc.xi or got["taupath"] < 1e-10)
            checked += 1
    assert checked >= 200, checked


@pytest.mark.parametrize("name", ["cfg1nf", "cfg1nfea", "cfg1mmnf"])
def test_non_forced_restatement_equals_the_oracle(name, scene):
    """a non-forced walk for every committed ray and every depth of non_forced_depths: equal to a partial sum (the walk goes on), its two
    neighbours, 0, and beyond the path (the packet escapes)"""
    sc = scene(name)
    assert not sc.forced
    checked = escaped = 0
    for r, k in W.golden_rays(SCENES[name]):
        path = sc.path(r, k)
        if path is None or len(path[0]) == 0:
            continue
        sums = W.partial_sums(sc, path)
        for depth in W.non_forced_depths(sums):
            got = W.non_forced(sc, path, depth)
            ref, cell, visits = sc.oracle(2, r, k, depth)
            assert got["mint"] == cell, (name, r, k, depth)
            assert got["visits"] == visits
            if cell < 0:
                escaped += 1
                continue
            assert same(got["sint"], ref[1]), (name, r, k, depth)
            if sc.ea:
                assert same(got["nint"], ref[2]), (name, r, k, depth)
            else:
                assert same(got["nint"], sc.dens[0][cell])
            checked += 1
        # a depth equal to a partial sum stops in a LATER segment than the depth just below it
        t = next((t for t in sums if t > 0.), None)
        if t is not None and sums[-1] > t:
            below, at = W.non_forced(sc, path, float(np.nextafter(t, -math.inf))), W.non_forced(sc, path, t)
            assert at["visits"] > below["visits"]
    assert checked >= 200 and escaped >= 10, (checked, escaped)


def test_restatement_on_a_synthetic_path():
    """the restatement itself, on a path written out by hand: zero-length segments, empty cells, the way to the grid"""
    class S:
        num_media, ea, forced, xi, wavelength = 1, False, True, 0.5, 1.
        mm = False
        sext, ssca, sabs = [2.], [1.], [1.]
        dens = [np.array([0., 1., 3., 0.])]
    path = (np.array([-1, 0, 1, 1, 2, 3]), np.array([5., 1., 2., 0., 1., 4.]))
    assert W.partial_sums(S, path) == [0., 0., 4., 4., 10., 10.]
    assert W.peel(S, path, 745.) == (10., 5)
    assert W.peel(S, path, 10.) == (math.inf, 4)            # tau >= taumax stops the walk
    assert W.peel(S, path, float(np.nextafter(10., 11.))) == (10., 5)
    assert W.peel(S, path, -math.inf) == (math.inf, 0)
    assert W.peel(S, None, 745.) == (0., 0)
    got = W.forced(S, path, 0., 0.5)
    assert (got["taupath"], got["tausample"], got["mint"], got["sint"], got["nint"], got["visits"], got["rewalks"]) == (10., 5., 2, 8. + (1. / 6.) * 1., 3., 4, 3)
    got = W.forced(S, path, 0., 2. ** -1074)                # the first segment with optical depth, behind an empty cell
    assert (got["mint"], got["sint"], got["rewalks"]) == (1, 6., 2)
    got = W.forced(S, path, 0., 1. - 2. ** -53)
    assert got["mint"] == 2 and 8.9 < got["sint"] <= 9. and got["rewalks"] == 3
    S.forced = False
    assert W.non_forced(S, path, 4.)["mint"] == 2           # equal to a partial sum: the walk goes on
    assert W.non_forced(S, path, float(np.nextafter(4., 0.)))["mint"] == 1
    assert W.non_forced(S, path, 10.) == dict(mint=-1, sint=None, nint=None, visits=5)
    assert W.non_forced(S, path, 0.)["mint"] == 1 and W.non_forced(S, path, 0.)["sint"] == 6.


def test_exponential_budget_follows_the_cancellation():
    """the error allowed on the exponential branch of the sampled depth: a few ulp where 1 - d keeps its bits, growing as d = u2 (1 - e^-taupath)
    shrinks, and no claim at all below 2^-53, where the formulation itself returns 0 or 2^-53"""
    cases = [(t, u) for t in (0.3, 1.7, 2.6, 60.) for u in (2. ** -53, 1e-9, 0.03, 0.25, 0.5, 0.77, 0.999)]
    exact, room, envelope = W.exponential_budget(cases)
    print("envelope of the restatement per binade of d:", ", ".join(f"{e}: {v:.2g}" for e, v in sorted(envelope.items())))
    for (t, u), e, r in zip(cases, exact, room):
        d = u * (1. - math.exp(-t))
        assert abs(-math.log(1. - d) - e) <= r
        if d >= 2. ** -8:
            assert r <= 1e-12 * e, (t, u, float(r / e))
        if d < 2. ** -53:
            assert r >= 0.5 * e


def test_field_contributions_sum_to_the_absorbed_luminosity(scene):
    """the restated radiation-field contributions of a pass-1 walk: within 1e-12 of their exact values, and sum over a path of
    sigma n x contribution = L (1 - e^-tau_path), the luminosity the path takes out of the packet"""
    import mpmath as mp
    sc = scene("cfg1")
    checked = 0
    for r, k in W.golden_rays("cfg1"):
        path = sc.path(r, k)
        if path is None or len(path[0]) == 0:
            continue
        parts = W.field_contributions(sc, path, 2.5)
        taupath = W.partial_sums(sc, path)[-1]
        if not taupath > 0.:
            continue
        for m, value, exact in parts:
            assert abs(mp.mpf(value) - exact) <= 1e-12 * exact
        taken = sum(mp.mpf(sc.sext[0]) * mp.mpf(float(sc.dens[0][m])) * exact for m, _, exact in parts)
        assert abs(taken - 2.5 * (1 - mp.exp(-mp.mpf(taupath)))) <= 1e-12 * taken
        checked += 1
    assert checked >= 30
