"""The references of tests/primitive_checks.py, checked on the CPU: the restatements of the scalar device functions against exact evaluations
of the same operations (mpmath) and against the mathematical functions behind them, the oracle's own copies against the restatements bit for
bit, the argument lists (every branch reached, either side of every border), and the acceptance rule on the restatements themselves.  What
the device functions return is checked against the same references by tests/test_gpu_primitives.py."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
import primitive_checks as P

U = 2.0 ** -53  # unit roundoff of a double


def cap(name, branch, inputs):
    """An upper bound of the envelope of (function, branch) from the conditioning of the operation -- not from what the restatement gives.
    A well-conditioned chain of n <= 16 correctly rounded operations and libm calls of < 1 ulp: 16 u (relative, or absolute for values of
    order one).  The ill-conditioned ones:
      * the Henyey-Greenstein kernel 1 + g^2 - 2 g cos is (1 - |g|)^2 at the peak and is formed from terms of order one: a rounding of u in
        it is a relative u / (1 - |g|)^2, which the value and the cone mean (through rootFar - rootNear) inherit: 16 u resp. 64 u over (1 - |g|)^2;
      * the HG cosine divides the rounding of 1 + g^2 - f^2 by 2 g, and f itself divides by 1 - g + 2 g X >= 1 - |g|: 8 u / min(|g|, 1 - |g|);
      * pow(1 + d x, 1 / d) raises the rounding of its base to the power 1 / d: 4 u (1 + 1 / |d|) with the smallest |d| of the branch, 1e-3;
      * directionAbout divides by sqrt(1 - kz^2): 16 u / sqrt(1 - kz^2), at most 16 u / 4.47e-3 in the general branch;
      * interpolateLogLog multiplies the rounding of the exponent by the exponent's size, |ln(f2 / f1)| <= 32 over the list: 64 u;
      * the peel-off depth log(L) + 745 is a sum near 745: 2 ulp(745)."""
    g = np.abs(inputs[:, 0]).max() if len(inputs) else 0.
    if name == "hg_value" or (name == "phase_value" and branch == "value"):
        return 16 * U / (1. - g) ** 2
    if name in ("hg_cone_mean", "phase_value"):
        return 64 * U / (1. - g) ** 2
    if name == "hg_cosine":
        return 8 * U / min(np.abs(inputs[:, 0]).min(), 1. - g)
    if name == "generalized_exp" and branch == "pow":
        return 4 * U * (1. + 1. / 1e-3)
    if name == "direction_about" and branch.startswith("general"):
        return 16 * U / math.sqrt((1. - 0.99999) * (1. + 0.99999))
    if name == "interpolate_loglog":
        return 64 * U
    if name == "peel_taumax":
        return 2 * math.ulp(745.)
    return 16 * U


@pytest.mark.parametrize("name", list(P.FUNCTIONS))
def test_restatement_against_the_exact_evaluation(name):
    """the envelope of every (function, branch): measured, printed, below the bound that the conditioning of the operation gives; and every
    listed tuple is admissible by the acceptance rule for the restatement alone"""
    inputs = P.FUNCTIONS[name].inputs()
    labels = np.array(P.branches(name, inputs))
    envelope = P.envelopes(name)
    kind = "absolute" if P.FUNCTIONS[name].absolute else "relative"
    for branch in sorted(envelope):
        rows = inputs[labels == branch]
        bound = cap(name, branch, rows)
        print(f"envelope {name:22s} {branch:32s} {envelope[branch]:9.2e} {kind} over {len(rows):4d} tuples (bound {bound:.2e})")
        assert envelope[branch] <= bound, (name, branch, envelope[branch], bound)
    values = P.restated(name, inputs)
    assert np.isfinite(values[np.isfinite(inputs).all(axis=1) & (labels != "dead")]).all()
    assert P.inadmissible(name, inputs, values) == []


def test_every_branch_is_reached():
    want = {"hg_cone_mean": {f"{fold}|g={g:.12g}" for fold in ("forward", "general", "backward") for g in (0.95000000000000006661, 0.97, 0.999, 0.999999)},
            "random_direction": {"pole", "general"},
            "lambert_lower_branch": {"zero", "series", "iterated", "asymptotic"},
            "generalized_exp": {"exp", "expansion", "pow"},
            "interpolate_loglog": {"zero", "log"},
            "lnmean": {"zero", "series", "quotient"},
            "peel_taumax": {"dead", "log"}}
    for name, branches in want.items():
        inputs = P.FUNCTIONS[name].inputs()
        assert branches <= set(P.branches(name, inputs)), (name, branches - set(P.branches(name, inputs)))
    labels = set(P.branches("direction_about", P.inputs_direction_about()))
    assert {"pole|kz=1", "general|kz=0", "general|kz=0.99999000000000005", "general|kz=interior"} <= labels and len(labels) == 6
    # g = 0.95 itself takes the plain value, the next double the cone mean; the two differ, so that a wrong switch shows
    up = math.nextafter(0.95, 1.)
    for g in (0.95, -0.95):
        assert P.branch_phase_value(g, 0.3) == "value" and P.branch_phase_value(math.copysign(up, g), 0.3) != "value"
        assert P.restate_phase_value(g, 0.3) == P.restate_hg_value(g, 0.3) != P.restate_hg_cone_mean(g, 0.3)
    # the isotropic branch of the scattering event: |g| < 1e-6
    flags = {g: P.restate_hg_cosine(g, 0.5)[1] for g in (1e-6, math.nextafter(1e-6, 0.), -1e-6, -math.nextafter(1e-6, 0.))}
    assert flags == {1e-6: 0., math.nextafter(1e-6, 0.): 1., -1e-6: 0., -math.nextafter(1e-6, 0.): 1.}
    # the cosines of the HG sampler leave [-1, 1] at some of the listed tuples, by no more than 1e-9
    cosines = P.restated("hg_cosine", P.inputs_hg_cosine())[:, 0]
    assert (np.abs(cosines) > 1.).any() and np.abs(cosines).max() < 1. + 1e-9
    # either side of the two switches of the Lambert function, and of those of lnmean and the generalised exponential, is in the lists
    z = P.inputs_lambert()[:, 0]
    for switch in (3e-3 - P.INVERSE_E, -1e-6):
        assert {P.step(switch, -1), switch, P.step(switch, 1)} <= set(z)
    assert {P.branch_lambert(P.step(-1e-6, -1)), P.branch_lambert(-1e-6)} == {"iterated", "asymptotic"}
    p = set(P.inputs_generalized_exp()[:, 0])
    for d in (1e-3, -1e-3):
        near = [P.step(1. - d, n) for n in range(-2, 3)]
        assert set(near) <= p and {P.branch_generalized_exp(q, 1.) for q in near} == {"expansion", "pow"}
    assert 1. in p and {1. - d for d in P.GEXP_DEFICIT} <= p


def test_lambert_iteration_converges_at_every_listed_argument():
    """no listed argument leaves the tenth Halley round without meeting the criterion (the reference would raise "no convergence")"""
    rounds = {}
    for z in P.inputs_lambert()[:, 0]:
        w, branch, n, converged = P.lambert_trace(float(z))
        assert converged, (z, w)
        rounds[branch] = max(rounds.get(branch, 0), n)
    print("Halley rounds at most:", rounds)
    assert rounds["iterated"] <= 9 and rounds["asymptotic"] <= 9


def test_operations_against_the_mathematical_functions():
    """the operations as the reference formulates them against the functions behind them, within the truncation of the formulation: measured
    per branch (printed), and bounded from the formulation"""
    mp = P._mp()
    worst = {}

    def note(key, err, bound, what):
        worst[key] = max(worst.get(key, 0.), float(err))
        assert err <= bound, (key, what, float(err), float(bound))

    # Lambert W_-1: the Halley iteration stops below a relative correction of 1e-12 (and is then far closer); the series stops at the twelfth
    # power of sqrt(z + 1/e) <= sqrt(3e-3) with coefficients below 60, and sees z + 1/e with the rounding of the constant 1/e: 1.3e-17
    for z in P.inputs_lambert()[:, 0]:
        w, branch, _, _ = P.lambert_trace(float(z))
        if branch == "zero" or z <= -1. / math.e:
            continue   # (W(0) = -infinity stands for -DBL_MAX; the double -1/e lies below the branch point by the rounding of the constant)
        err = abs(P.exact_lambert(float(z)) - P.math_lambert(float(z)))
        q = float(z) + P.INVERSE_E
        bound = 2.4 * math.sqrt(1.3e-17) + 60. * q ** 6 if branch == "series" else 2e-12 * (1. + abs(w))
        note(("lambert", branch), err, bound, z)
    # generalised exponential: the expansion stops behind the third order in d = 1 - p; the fourth-order term of exp(ln(1 + d x) / d - x) is
    # d^4 (x^5/5 + x^6/8 + x^6/18 + x^7/24 + x^8/384), and the next ones are smaller by |d x| <= 3e-3 each: twice that term
    for p, x in P.inputs_generalized_exp():
        branch = P.branch_generalized_exp(float(p), float(x))
        truth = P.math_generalized_exp(float(p), float(x))
        err = abs(P.exact_generalized_exp(float(p), float(x)) - truth) / truth
        a, d = abs(float(x)), abs(1. - float(p))
        bound = 2. * d ** 4 * (a ** 5 / 5 + a ** 6 * (1 / 8 + 1 / 18) + a ** 7 / 24 + a ** 8 / 384) + 1e-45 if branch == "expansion" else 1e-45   # (1e-45: the 50 digits)
        note(("generalized_exp", branch), err, bound, (p, x))
    # logarithmic mean: the series of x / ln(1 + x) stops behind x^5 / 6, the next term is x^6 / 7 with x < 1e-3; the quotient is handed two
    # logarithms rounded to half an ulp each
    for x1, x2, l1, l2 in P.inputs_lnmean():
        branch = P.branch_lnmean(*(float(v) for v in (x1, x2, l1, l2)))
        if branch == "zero":
            continue
        truth = P.math_lnmean(float(x1), float(x2))
        err = abs(P.exact_lnmean(*(float(v) for v in (x1, x2, l1, l2))) - truth) / truth
        ratio = max(x1, x2) / min(x1, x2) - 1.
        # (the 50 digits of the logarithm of a ratio next to 1 leave 1e-50 / (ratio - 1) of the mean)
        bound = 2. * ratio ** 6 / 7. + 1e-47 / max(ratio, U) if branch == "series" else (math.ulp(l1) + math.ulp(l2)) / 2. / abs(l2 - l1) * 1.01
        note(("lnmean", branch), err, bound, (x1, x2))
    # cone mean: the operation IS the closed-form integral; the exact evaluation differs from it by the rounding of pi in the half angle and in
    # the fold (relative 1.2e-16 in an angle), which the cancellation next to the peak multiplies like every other rounding: u / (1 - |g|)^2
    for g in P.CONE_G:
        for c in P.CONE_COS:
            truth = P.math_hg_cone_mean(g, c)
            err = abs(P.exact_hg_cone_mean(g, c) - truth) / truth
            note(("hg_cone_mean", f"g={abs(g):.6g}"), err, 64 * U / (1. - abs(g)) ** 2, (g, c))
    # ... and the antiderivative behind math_hg_cone_mean is the integral of the phase function (a quadrature, at a few tuples)
    for g, c in ((0.97, 0.3), (-0.97, 0.3), (0.95, math.cos(0.02)), (0.999, -1.)):
        gm, half = mp.mpf(g), 4 * mp.pi / 180
        theta = mp.acos(mp.mpf(c))
        density = lambda mu: (1 - gm * gm) / (1 + gm * gm - 2 * gm * mu) ** mp.mpf(1.5)   # noqa: E731
        lo, hi = mp.cos(theta + half), mp.cos(theta - half)
        if theta < half:
            mean = (mp.quad(density, [hi, 1]) + mp.quad(density, [lo, 1])) / (2 - hi - lo)
        elif theta > mp.pi - half:
            mean = (mp.quad(density, [-1, hi]) + mp.quad(density, [-1, lo])) / (2 + hi + lo)
        else:
            mean = mp.quad(density, [lo, hi]) / (hi - lo)
        assert abs(mean - P.math_hg_cone_mean(g, c)) <= mp.mpf(10) ** -25 * mean, (g, c)
    for key in sorted(worst):
        print(f"truncation {key[0]:18s} {key[1]:14s} {worst[key]:.2e}")


ORACLE_COPIES = ["hg_value", "hg_cone_mean", "phase_value", "dipole_value", "random_direction", "direction_about", "lambert_lower_branch", "generalized_exp",
                 "interpolate_loglog", "lnmean"]


def oracle_evaluate(name, inputs):
    from skirt9_amd.engine import DEVICE_FUNCTIONS
    L = O.lib()
    L.oracle_evaluate.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    a = np.ascontiguousarray(inputs, dtype=np.float64)
    out = np.full((a.shape[0], P.FUNCTIONS[name].outputs), np.nan)
    assert L.oracle_evaluate(DEVICE_FUNCTIONS[name], a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p)) == 0
    return out


@pytest.mark.parametrize("name", ORACLE_COPIES)
def test_oracle_copies_equal_the_restatements_bit_for_bit(name):
    """the oracle's gexp, lambertW1, lnmean, meanHG, valueHG, interpolateLogLog and direction functions run the same libm as the restatements"""
    inputs = P.FUNCTIONS[name].inputs()
    got, want = oracle_evaluate(name, inputs), P.restated(name, inputs)
    differ = np.flatnonzero((P.bits(got) != P.bits(want)).any(axis=1))
    assert differ.size == 0, (name, differ.size, inputs[differ[0]], got[differ[0]], want[differ[0]])


def test_oracle_has_no_copy_of_the_other_functions():
    from skirt9_amd.engine import DEVICE_FUNCTIONS
    L = O.lib()
    L.oracle_evaluate.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    one = np.ones(8)
    for name in set(DEVICE_FUNCTIONS) - set(ORACLE_COPIES):
        assert L.oracle_evaluate(DEVICE_FUNCTIONS[name], one.ctypes.data_as(C.c_void_p), 1, one.ctypes.data_as(C.c_void_p)) == -2
    assert L.oracle_evaluate(13, one.ctypes.data_as(C.c_void_p), 1, one.ctypes.data_as(C.c_void_p)) == -1
    assert L.oracle_evaluate(0, None, 1, one.ctypes.data_as(C.c_void_p)) == -1


def test_table_searches_against_searchsorted():
    """the three searches as written (the loop of NR::locateBasic) against numpy.searchsorted, on every table and probe of the GPU test"""
    for key, nodes in P.locate_tables().items():
        x = P.locate_probes(nodes)
        for kind in ("locate", "locate_clip", "locate_basic"):
            want = np.array([P.restate_locate(kind, nodes, float(v)) for v in x], dtype=np.int32)
            assert np.array_equal(P.reference_locate(kind, nodes, x), want), (key, kind)
        n = len(nodes)
        assert P.restate_locate("locate", nodes, float(nodes[-1])) == n - 2 and P.restate_locate("locate_basic", nodes, float(nodes[-1])) == n - 1
        assert P.restate_locate("locate_clip", nodes, float(nodes[0]) - 1.) == 0 and P.restate_locate("locate", nodes, float(nodes[0]) - 1.) == -1
        assert P.restate_locate("locate_clip", nodes, math.inf) == n - 2


def synthetic_instruments():
    """instrument values as pmc_tune_instrument returns them: a rotated, offset, non-square frame with an aperture and a redshift, and an
    axis-aligned one (whose projection is exact)"""
    def angles(theta, phi, omega):
        return dict(costheta=math.cos(theta), sintheta=math.sin(theta), cosphi=math.cos(phi), sinphi=math.sin(phi), cosomega=math.cos(omega), sinomega=math.sin(omega))
    pc = 3.0856775814913673e16
    border = np.array([1e-7, 2e-7, 2e-7, 3.5e-7, 3.5e-7, 9e-7])   # two bins with a gap between them and one that touches the next
    ellv = np.array([-1, 0, -1, 1, 2, 2, -1], dtype=np.int32)
    tilted = dict(angles(1.0471975511965976, 0.5235987755982988, 0.3490658503988659), nxp=16, nyp=12, xpsiz=1250. * pc, ypsiz=10000. / 12. * pc,
                  xpmin=-9000. * pc, ypmin=-5500. * pc, aperture_r2=(0.4 * pc) ** 2, zp1=1.5, border=border, ellv=ellv)
    aligned = dict(costheta=1., sintheta=0., cosphi=1., sinphi=0., cosomega=1., sinomega=0., nxp=12, nyp=12, xpsiz=1000. * pc, ypsiz=1000. * pc, xpmin=-6000. * pc,
                   ypmin=-4000. * pc, aperture_r2=(7. * pc) ** 2, zp1=1., border=border, ellv=ellv)
    centred = dict(tilted, nxp=24, nyp=24, xpsiz=40000. / 24. * pc, ypsiz=40000. / 24. * pc, xpmin=-20000. * pc, ypmin=-20000. * pc)   # (a border at 0)
    return {"tilted": tilted, "aligned": aligned, "centred": centred}


@pytest.mark.parametrize("which", ["tilted", "aligned", "centred"])
def test_detector_positions_reach_either_side_of_every_border(which):
    I = synthetic_instruments()[which]
    r = P.frame_positions(I)
    i, j = P.pixel_coordinates(I, r)
    for coordinate, count in ((i, I["nxp"]), (j, I["nyp"])):
        for border in range(count + 1):
            assert (coordinate == border - 1).any() and (coordinate == border).any(), (which, border)
        assert (coordinate < -1e5).any() and (coordinate > 1e5).any()
    pixel = P.reference_pixel(I, r)
    # the reference as the scalar code reads, position by position; and what truncation in place of floor would have given differs
    for n in range(0, len(r), 7):
        xp, yp, _, _ = P.detector_plane(I, r[n:n + 1])
        a, b = math.floor((xp[0] - I["xpmin"]) / I["xpsiz"]), math.floor((yp[0] - I["ypmin"]) / I["ypsiz"])
        assert pixel[n] == (-1 if a < 0 or a >= I["nxp"] or b < 0 or b >= I["nyp"] else a + I["nxp"] * b)
    truncated = np.trunc((P.detector_plane(I, r)[0] - I["xpmin"]) / I["xpsiz"])
    assert ((truncated == 0) & (i == -1) & (j >= 0) & (j < I["nyp"])).any()
    assert set(np.unique(pixel)) >= {-1, 0, I["nxp"] - 1, I["nxp"] * (I["nyp"] - 1), I["nxp"] * I["nyp"] - 1}
    # the aperture: squared radii on either side of aperture_r2
    a = P.aperture_positions(I)
    _, _, xpp, ypp = P.detector_plane(I, a)
    radius2 = xpp * xpp + ypp * ypp
    assert (radius2 > I["aperture_r2"]).any() and (radius2 < I["aperture_r2"]).any() and (np.abs(radius2 / I["aperture_r2"] - 1.) < 8 * U).any()
    inside = P.reference_inside(I, a)
    assert inside[0] == 1 and inside[1] == 0 and inside[2] == 0 and np.array_equal(inside == 0, radius2 > I["aperture_r2"])
    if which == "aligned":
        assert (radius2 == I["aperture_r2"]).any() and inside[radius2 == I["aperture_r2"]].all()
    assert P.reference_inside(dict(I, aperture_r2=0.), a).all()
    # the wavelength bins: either side of every border, in the observer's frame
    lam = P.bin_wavelengths(I)
    seen = lam * I["zp1"]
    for b in I["border"]:
        assert (seen < b).any() and (seen == b).any() and (seen > b).any()
    ell = P.reference_bin(I, lam)
    assert ell[0] == -1 and ell[1] == -1 and set(ell) == {-1, 0, 1, 2}
    for n in range(len(lam)):   # (std::upper_bound as written)
        count = sum(1 for b in I["border"] if b <= seen[n])
        assert ell[n] == I["ellv"][count]


@pytest.mark.parametrize("kind", [P.ANGULAR_LASER, P.ANGULAR_CONICAL, P.ANGULAR_NETZER])
def test_angular_directions_reach_either_side_of_the_switch(kind):
    axis = np.array([0.36, -0.48, 0.8])
    cos_delta = math.cos(0.6)
    k = P.angular_directions(kind, axis, cos_delta)
    p = np.array([P.restate_angular_probability(kind, axis, cos_delta, row) for row in k])
    cosines = axis[0] * k[:, 0] + axis[1] * k[:, 1] + axis[2] * k[:, 2]   # (in the function's order)
    if kind == P.ANGULAR_LASER:
        assert set(p) == {0., math.inf} and p[0] == math.inf and p[1] == 0.
        assert ((cosines > 0.99999 - 1e-14) & (p == 0.)).any() and ((cosines < 0.99999 + 1e-14) & (p > 0.)).any()
        assert (cosines == 0.99999).any() and not p[cosines == 0.99999].any()   # (on the switch: not beyond it)
    elif kind == P.ANGULAR_CONICAL:
        assert set(p) == {0., 1.0 / (1.0 - cos_delta)} and p[0] > 0. and p[1] > 0.
        for edge in (cos_delta, -cos_delta):
            near = np.abs(cosines - edge) < 1e-14
            assert (near & (p == 0.)).any() and (near & (p > 0.)).any()
            assert (cosines == edge).any() and not p[cosines == edge].any()
    else:
        assert p[0] == (6. / 7.) * 3. and p[1] == p[0] and (p >= 0.).all()   # (2 cos^2 + |cos|) 6/7: the sign makes it even
        assert (cosines[2:] < 0.).any() and (cosines[2:] > 0.).any()


def test_oracle_census_counts_the_branches():
    """oracle_census (tests/primitive_census.py, the table of DESIGN.md section 2) counts what the branch functions of the restatements say"""
    from primitive_census import census
    census()
    expected = [0] * 10
    for name, first, marks in (("hg_cone_mean", 0, {"forward": 1, "backward": 2}), ("lambert_lower_branch", 3, {"series": 1, "asymptotic": 2}),
                               ("generalized_exp", 6, {"expansion": 1}), ("lnmean", 8, {"series": 1})):
        inputs = P.FUNCTIONS[name].inputs()
        oracle_evaluate(name, inputs)
        labels = [label.split("|")[0] for label in P.branches(name, inputs)]
        expected[first] += len(labels)
        for label, offset in marks.items():
            expected[first + offset] += labels.count(label)
    assert census() == expected and min(expected) > 0
    assert census() == [0] * 10
