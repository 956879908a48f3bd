"""What the walk kernels leave in a slot after one walk, restated from the reference's (m, ds) sequence of the walk's path (oracle_trace_ray) in
scalar Python doubles, in the kernels' operation order (pmc_walk.inc segmentDepth, mediaSegment, sampleForcedDepth, storeInteraction,
storeWalkEnd; prepareWalk's stop value of a peel-off walk).  Every operation here is one IEEE double operation, as in the kernels, which are built
with -ffp-contract=off: the results are compared bit for bit.  The only libm calls of the walks -- the log of the peel-off stop value and the exp
and log of the exponential branch of the sampled depth -- enter as arguments (taumax, tausample).

tests/test_walk_checks.py holds this restatement to the oracle's own path code (oracle_walk_result); tests/test_gpu_walk_kernels.py holds the
kernels to it.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O

INF = math.inf
GRID_CARTESIAN, GRID_OCTREE, GRID_VORONOI, GRID_BINTREE = 1, 2, 3, 4  # include/pmc.h PMC_GRID_*


def bits(x):
    """the bit patterns of doubles (an array of uint64): what `bit for bit` compares"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Scene:
    """What the walks read of a set-up Simulation: options, observers, and per medium component the cross sections at `wavelength` (default:
    the scene's one wavelength) and the cell densities"""

    def __init__(self, sim, wavelength=None):
        L = O.lib()
        L.oracle_walk_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_walk_medium.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_walk_result.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        self.sim = sim
        info = np.zeros(5, dtype=np.int32)
        xi = C.c_double(0.)
        assert L.oracle_walk_scene(sim.scene, info.ctypes.data, C.byref(xi), None, None) == 0
        self.num_instruments, self.num_media = int(info[0]), int(info[1])
        self.forced, self.ea, self.rf = bool(info[2]), bool(info[3]), bool(info[4])
        self.xi = xi.value
        L.oracle_walk_field_bin.argtypes = [C.c_void_p, C.c_double]
        self.kobs = np.zeros((self.num_instruments, 3))
        leader = np.zeros(self.num_instruments, dtype=np.int32)
        assert L.oracle_walk_scene(sim.scene, info.ctypes.data, C.byref(xi), self.kobs.ctypes.data, leader.ctypes.data) == 0
        self.leaders = [i for i in range(self.num_instruments) if leader[i]]
        from skirt9_amd.host import SceneHead
        self.num_cells = int(SceneHead.from_address(int(sim.scene)).grid.num_cells)
        self.grid_kind = int(SceneHead.from_address(int(sim.scene)).grid.kind)
        lam0 = C.c_double(0.)
        sec = np.zeros(3)
        assert L.oracle_walk_medium(sim.scene, 0, 1e-6, sec.ctypes.data, None, C.byref(lam0), None) == 0
        # (a scene whose first source is not oligochromatic has no wavelength of its own: the walks run at the one given, or at 0.55 micron)
        self.wavelength = float(wavelength) if wavelength is not None else lam0.value if lam0.value > 0. else 5.5e-7
        self.sext, self.ssca, self.sabs, self.dens, self.index = [], [], [], [], []
        for h in range(self.num_media):
            dens = np.zeros(self.num_cells)
            index = C.c_int32(0)
            assert L.oracle_walk_medium(sim.scene, h, self.wavelength, sec.ctypes.data, dens.ctypes.data, None, C.byref(index)) == 0
            self.index.append(int(index.value))
            self.sext.append(float(sec[0])), self.ssca.append(float(sec[1])), self.sabs.append(float(sec[2]))
            self.dens.append(dens)

    @property
    def field_bin(self):
        """the bin of the scene's wavelength in the grid of the stored radiation field (-1: outside)"""
        return int(O.lib().oracle_walk_field_bin(self.sim.scene, self.wavelength))

    @property
    def mm(self):
        return self.num_media > 1

    def path(self, r, k, cap=4096):
        """the reference's (m, ds) sequence of the path from r along k, or None when it has `cap` segments or more"""
        m, ds = O.trace_ray(self.sim, r, k, cap)
        return None if len(m) >= cap else (m, ds)

    def oracle(self, kind, r, k, value):
        """oracle_walk_result: kind 0 peel-off (value = W), 1 forced (value = the sampled depth), 2 non-forced (value = the drawn depth);
        returns (out[3], cell, visits)"""
        r, k = np.ascontiguousarray(r, dtype=np.float64), np.ascontiguousarray(k, dtype=np.float64)
        out = np.zeros(3)
        cell, visits = C.c_int32(0), C.c_uint64(0)
        rc = O.lib().oracle_walk_result(self.sim.scene, kind, r.ctypes.data, k.ctypes.data, self.wavelength, float(value), out.ctypes.data,
                                        C.byref(cell), C.byref(visits))
        assert rc == 0, rc
        return out, int(cell.value), int(visits.value)


def load_scene(name, tmp_path, num_packets=1000):
    """the Scene of tests/ski/<name>.ski; `<base>@<depth>`: the variant of <base> whose material normalization has that optical depth (the
    committed scenes are optically thin: a peel-off walk stops inside a path only where the path has an optical depth of 15 or more)"""
    from conftest import ski
    from scene_variants import with_optical_depth
    from skirt9_amd.host import Simulation
    base, _, depth = name.partition("@")
    path = with_optical_depth(tmp_path, base, int(depth)) if depth else ski(base + ".ski")
    return Scene(Simulation(path, num_packets=num_packets).setup())


def _segment(sc, m, ds, tau, tabs, apart, force):
    """segmentDepth / mediaSegment: the optical depth(s) at the end of a segment of length ds through cell m from those at its start.  apart:
    a propagation walk (explicit absorption sums scattering and absorption depths apart), else a peel-off walk (extinction)"""
    if m < 0:
        return tau, tabs  # (the way to the grid: no medium)
    if sc.mm:
        for h in range(sc.num_media):
            n = float(sc.dens[h][m])
            if sc.ea and apart:
                ns = n * ds
                tau = tau + sc.ssca[h] * ns
                tabs = tabs + sc.sabs[h] * ns
            else:
                tau = tau + sc.sext[h] * n * ds
        return tau, tabs
    dens = float(sc.dens[0][m])
    if sc.ea and apart:
        ns = dens * ds
        return (tau + sc.ssca[0] * ns) if force else (tau + sc.ssca[0] * dens * ds), tabs + sc.sabs[0] * ns
    return tau + sc.sext[0] * dens * ds, 0.


def partial_sums(sc, path, apart=True):
    """the optical depth after every segment of the path (a list, one per segment of (m, ds)), on the depth the walk samples"""
    tau, tabs, sums = 0., 0., []
    for m, ds in zip(*path):
        tau, tabs = _segment(sc, int(m), float(ds), tau, tabs, apart, sc.forced)
        sums.append(tau)
    return sums


def peel_taumax(ppW, wavelength):
    """peelTaumax with the HOST's log: -inf flags a dead packet"""
    lum = ppW / wavelength
    return -INF if lum <= 0 else math.log(lum) + 745


def peel(sc, path, taumax):
    """a peel-off walk: (ptau, cell visits).  taumax: the stop value (MediumSystem::getExtinctionOpticalDepth), -inf for a packet without
    luminosity.  path None or empty: the walk misses the grid"""
    if taumax == -INF:
        return INF, 0
    if path is None or len(path[0]) == 0:
        return 0., 0
    target = np.nextafter(taumax, -INF)  # (the kernels test tau > target only)
    tau, visits = 0., 0
    for m, ds in zip(*path):
        if int(m) < 0:
            continue
        tau1, _ = _segment(sc, int(m), float(ds), tau, 0., False, sc.forced)
        visits += 1
        if tau1 > target:
            return INF, visits
        tau = tau1
    return tau, visits


def sample_forced_depth(sc, taupath, u1, u2):
    """sampleForcedDepth with the HOST's exp and log: (depth, exact) -- exact: the depth is u2 * taupath, one multiplication"""
    if (sc.xi != 0. and u1 < sc.xi) or taupath < 1e-10:
        return u2 * taupath, True
    return -math.log(1.0 - u2 * (1.0 - math.exp(-taupath))), False


def _interaction(sc, m, ds, s, tau, tabs, target, force):
    """storeInteraction in the segment (m, ds) that starts at distance s with the depths tau, tabs: (mint, sint, nint)"""
    tau1, tabs1 = _segment(sc, m, ds, tau, tabs, True, force)
    f = (target - tau) / (tau1 - tau)
    sint = s + f * ((s + ds) - s)
    if sc.ea and (sc.mm or force):
        nint = tabs + f * (tabs1 - tabs)
    elif sc.ea:
        nint = target * sc.sabs[0] / sc.ssca[0]
    else:
        nint = float(sc.dens[0][m])
    return m, sint, nint


def propagate(sc, path, target, force):
    """a pass-2 walk (force) or a non-forced walk up to `target` over the path: dict(mint, sint, nint, steps) -- mint -1: no interaction; steps:
    the segments the walk counts (forced: those with ds > 0 up to the one it stops in; not forced: every segment)"""
    tau, tabs, s, lastm, steps = 0., 0., 0., -1, 0
    for m, ds in zip(*path):
        m, ds = int(m), float(ds)
        if m < 0:
            s = s + ds
            continue
        tau1, tabs1 = _segment(sc, m, ds, tau, tabs, True, force)
        if tau1 > target:
            mint, sint, nint = _interaction(sc, m, ds, s, tau, tabs, target, force)
            return dict(mint=mint, sint=sint, nint=nint, steps=steps + 1)
        tau, tabs, s = tau1, tabs1, s + ds
        if ds > 0. or not force:
            lastm, steps = m, steps + 1
    if force and lastm >= 0:  # storeWalkEnd: the interaction point beyond the last segment
        return dict(mint=lastm, sint=s, nint=tabs if sc.ea else float(sc.dens[0][lastm]), steps=steps)
    return dict(mint=-1, sint=None, nint=None, steps=steps)


def forced(sc, path, u1, u2, tausample=None):
    """a forced propagation walk, both passes: dict(mint, sint, nint, taupath, tausample, exact, visits, rewalks).  tausample: the depth to use
    instead of the restated one (the device's, on the exponential branch).  A path without optical depth: mint -1 and nothing else"""
    if path is None or len(path[0]) == 0:
        return dict(mint=-1, taupath=None, visits=0, rewalks=0)
    sums = partial_sums(sc, path)
    visits = sum(1 for m, ds in zip(*path) if int(m) >= 0 and float(ds) > 0.)
    taupath = sums[-1]
    if not taupath > 0.:
        return dict(mint=-1, taupath=None, visits=visits, rewalks=0)
    depth, exact = sample_forced_depth(sc, taupath, u1, u2)
    if tausample is not None:
        depth = float(tausample)
    res = propagate(sc, path, depth, True)
    res.update(taupath=taupath, tausample=depth, exact=exact, visits=visits, rewalks=res.pop("steps"))
    return res


def non_forced(sc, path, depth):
    """a non-forced propagation walk up to the drawn depth: dict(mint, sint, nint, visits)"""
    if path is None or len(path[0]) == 0:
        return dict(mint=-1, visits=0)
    res = propagate(sc, path, float(depth), False)
    res["visits"] = res.pop("steps")
    return res


# ---- the cases both test modules run: rays, starts of peel-off walks, stop values

def golden_rays(name):
    """the committed rays of tests/golden/<name>_rays.txt: a list of (r, k)"""
    from conftest import golden
    rows = [[float.fromhex(t) for t in line.split()] for line in open(golden(name + "_rays.txt")) if line.strip()]
    return [(np.array(row[:3]), np.array(row[3:6])) for row in rows]


def grid_box(sim):
    from skirt9_amd.host import SceneHead
    g = SceneHead.from_address(int(sim.scene)).grid
    return np.array([g.xmin, g.ymin, g.zmin]), np.array([g.xmax, g.ymax, g.zmax])


def grid_points(sim, count=24):
    """points of the grid on cell corners, edges and faces: dyadic fractions of the box (a tree's or a regular mesh's walls); on a Voronoi grid
    the midpoints between neighbouring sites, which lie on the cells' bisecting planes"""
    from skirt9_amd.host import SceneHead
    g = SceneHead.from_address(int(sim.scene)).grid
    lo, hi = grid_box(sim)
    points = []
    if g.site:
        step = max(1, g.num_cells // count)
        for a in range(0, g.num_cells, step):
            b = g.vnbr_list[g.vnbr_start[a]]
            if b >= 0:
                points.append(np.array([0.5 * (g.site[3 * a + q] + g.site[3 * b + q]) for q in range(3)]))
        return points[:count]
    fractions = [(0.5, 0.5, 0.5), (0.25, 0.5, 0.75), (0.5, 0.5, 0.3), (0.5, 0.3, 0.7), (0.125, 0.125, 0.125), (0.75, 0.25, 0.6), (0.375, 0.625, 0.5),
                 (0.5, 0.75, 0.75), (0.0625, 0.5, 0.9375), (0.3, 0.6, 0.5), (0.875, 0.875, 0.125), (0.5, 0.4375, 0.5625), (0., 0.5, 0.5),
                 (1., 1., 1.), (0.5, 0., 0.25), (0.25, 0.25, 1.)]
    return [lo + np.array(f) * (hi - lo) for f in fractions][:count]


def peel_positions(sc, rays, instrument):
    """starts of peel-off walks towards the observer of `instrument`: every ray's start; P - t k_obs for the grid points P (t: a quarter of the
    box and several boxes, so that starts lie inside and outside the grid); starts beside the grid whose line of sight misses it"""
    lo, hi = grid_box(sc.sim)
    size = float(np.max(hi - lo))
    kobs = sc.kobs[instrument]
    side = np.cross(kobs, [0.3, -0.5, 0.81])
    side /= np.linalg.norm(side)
    out = [r for r, _ in rays]
    for j, P in enumerate(grid_points(sc.sim)):
        out.append(P - (0.25 * size if j % 2 else 3. * size) * kobs)
        out.append(P.copy())
    centre = 0.5 * (lo + hi)
    out.append(centre + 2. * size * side - 3. * size * kobs)  # misses the grid
    out.append(centre + 2. * size * kobs)                     # behind the grid: nothing towards the observer
    return out


FORCED_U2 = [2. ** -1074, 2. ** -53] + [q / 16. for q in range(1, 16)] + [1. - 2. ** -53]


def non_forced_depths(sums):
    """the drawn depths that probe a path with the partial sums `sums`: 0, every distinct positive partial sum with its two neighbours, and a
    depth beyond the path"""
    depths = [0.]
    for t in sorted(set(t for t in sums if t > 0.)):
        depths += [float(np.nextafter(t, -INF)), t, float(np.nextafter(t, INF))]
    depths.append((sums[-1] if sums else 0.) * 2. + 1.)
    return depths


def peel_weight_between(sc, sums, taumax_of):
    """a peel-off weight whose stop value lies midway between two partial sums of the path, so that the walk stops inside it: (ppW, index of the
    first partial sum above the stop value), or None.  The weight is lambda exp(t - 745) for the midpoint t: a positive double only for t above
    745 - 744.4 + ln(1 / lambda), about 15 at optical wavelengths, and coarsely spaced up to about 51 (subnormal weights), so only a path
    with that much optical depth has one; a pair of sums that the weight's stop value does not separate is passed over.  No partial sum lies
    within 1e-6 relative of the stop value (asserted): the last bits of a log cannot move the outcome.  taumax_of(ppW): the stop value of a
    weight"""
    distinct = sorted(set(t for t in sums if t > 0.))
    for a, b in zip(distinct, distinct[1:]):
        t = 0.5 * (a + b)
        ppW = sc.wavelength * math.exp(t - 745.)
        if ppW <= 0. or not a < taumax_of(ppW) < b or (b - a) <= 8e-6 * t:
            continue
        stop = taumax_of(ppW)
        if min(stop - a, b - stop) <= 2e-6 * stop:
            continue
        assert all(abs(x - stop) > 1e-6 * stop for x in sums), (sums, stop)
        return ppW, next(i for i, x in enumerate(sums) if x > stop)
    return None


# ---- the radiation field a pass-1 walk stores (rfSegment, pmc_walk.inc; MonteCarloSimulation::storeRadiationField)

def field_contributions(sc, path, lum):
    """what the pass-1 walk of a packet of luminosity lum over the path adds to the radiation field: a list of (cell, value, exact) per segment
    with ds > 0 -- value: L lnmean(e^-tau1, e^-tau0) ds restated in the kernels' operation order with the host's exp; exact: the same
    quantity, L (e^-tau0 - e^-tau1) / (tau1 - tau0) ds, in 200-bit arithmetic from the same partial sums tau0, tau1 (doubles, taken as they
    are)"""
    import mpmath as mp
    from primitive_checks import restate_lnmean
    mp.mp.prec = 200
    out, tau, tabs, ext_beg = [], 0., 0., 1.
    for m, ds in zip(*path):
        m, ds = int(m), float(ds)
        if m < 0:
            continue
        tau1, tabs1 = _segment(sc, m, ds, tau, tabs, True, True)
        if ds > 0.:
            ln_end, ln_beg = (-(tau1 + tabs1), -(tau + tabs)) if sc.ea else (-tau1, -tau)
            ext_end = math.exp(ln_end)
            value = lum * restate_lnmean(ext_end, ext_beg, ln_end, ln_beg) * ds
            a, b = mp.mpf(-ln_beg), mp.mpf(-ln_end)
            mean = mp.exp(-a) if a == b else (mp.exp(-a) - mp.exp(-b)) / (b - a)
            out.append((m, value, mp.mpf(lum) * mean * mp.mpf(ds)))
            ext_beg = ext_end
        tau, tabs = tau1, tabs1
    return out


def field_table(sc, walks, num_bins, ell):
    """the table that the pass-1 walks `walks` -- (path, luminosity) pairs -- leave in bin ell of an empty radiation field, and the error a device
    may have in every entry: (exact[num_cells] as floats, room[num_cells], envelope).  room = 4 x envelope x sum|v| + (n - 1) u sum|v| for the n
    contributions v of an entry: the envelope is the largest relative error of the restated contributions against their exact values, measured
    on these walks; (n - 1) u sum|v|, u = 2^-53, is what the order of n atomic additions can move a sum (the rule of the log kernels' tests)"""
    import mpmath as mp
    sums, mags, counts, envelope = {}, {}, {}, 0.
    for path, lum in walks:
        for m, value, exact in field_contributions(sc, path, lum):
            sums[m] = sums.get(m, mp.mpf(0)) + exact
            mags[m] = mags.get(m, mp.mpf(0)) + abs(exact)
            counts[m] = counts.get(m, 0) + 1
            if exact != 0:
                envelope = max(envelope, float(abs(mp.mpf(value) - exact) / abs(exact)))
    exact, room = np.zeros(sc.num_cells), np.zeros(sc.num_cells)
    for m in sums:
        exact[m] = float(sums[m])
        room[m] = float((4 * envelope + (counts[m] - 1) * 2. ** -53) * mags[m]) + math.ulp(exact[m])
    return exact, room, envelope


# ---- the exponential branch of the sampled depth: the one place where libm decides a walk's result

def exponential_budget(cases):
    """cases: (taupath, u2) pairs of the exponential branch of sampleForcedDepth.  Returns (exact, room, envelope): the depth -log(1 - u2 (1 - exp(-taupath)))
    of every case in 200-bit arithmetic, and the error allowed to a device: 4 x envelope x exact + 16 ulp(exact), as tests/primitive_checks.py
    allows a libm-bearing function.  The envelope is the largest relative error of THIS restatement (host exp and log) against the exact value,
    measured over the cases of the same class and over the 32 neighbouring values of u2 of each of them; a class is a binade of
    d = u2 (1 - exp(-taupath)), the parameter that decides how badly 1 - d cancels: the formulation loses log2(1 / d) bits whatever libm does
    (for d below 2^-53 it returns 0 or 2^-53 for a depth near d: an envelope of 1)"""
    import mpmath as mp
    mp.mp.prec = 200

    def exact_of(taupath, u2):
        return -mp.log(1 - mp.mpf(u2) * (1 - mp.exp(-mp.mpf(taupath))))

    def mine(taupath, u2):
        return -math.log(1.0 - u2 * (1.0 - math.exp(-taupath)))

    def binade(taupath, u2):
        return math.frexp(u2 * (1.0 - math.exp(-taupath)))[1]
    envelope = {}
    for taupath, u2 in cases:
        worst, v = envelope.get(binade(taupath, u2), 0.), u2
        for _ in range(16):
            v = float(np.nextafter(v, -INF))
        for _ in range(33):
            if 0. < v < 1.:
                e = exact_of(taupath, v)
                worst = max(worst, float(abs(mp.mpf(mine(taupath, v)) - e) / e))
            v = float(np.nextafter(v, INF))
        envelope[binade(taupath, u2)] = worst
    exact = [exact_of(taupath, u2) for taupath, u2 in cases]
    room = [4 * mp.mpf(envelope[binade(taupath, u2)]) * e + 16 * mp.mpf(math.ulp(float(e))) for (taupath, u2), e in zip(cases, exact)]
    return exact, room, envelope
