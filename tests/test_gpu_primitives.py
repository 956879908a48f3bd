"""The scalar device functions of the transition, launch and walk kernels at their edges: the product's own functions, run by the test aids of
include/pmc_tuning.h over the argument lists of tests/primitive_checks.py (one lane per tuple, at most 2^16 tuples per call), against the
references and by the acceptance rule of that module -- bit for bit where no libm call lies between input and output, else within four
times the envelope of the restatement plus 16 ulp of the exact value.  Every tuple must pass; the envelopes are measured at run time."""
import math

import numpy as np
import pytest

import primitive_checks as P
from conftest import ski
from skirt9_amd.host import Simulation

pytestmark = pytest.mark.gpu


def _context(name):
    from skirt9_amd.engine import Engine
    sim = Simulation(ski(name), num_packets=100).setup()
    return sim, Engine(sim.scene, 0)


@pytest.fixture(scope="module")
def tiny():
    """one tiny context for the scene-free functions"""
    sim, eng = _context("cfg1.ski")
    yield eng
    del eng, sim


def _show(bad):
    return f"{len(bad)} tuples miss the rule; the first: " + "; ".join(bad[:5])


@pytest.mark.parametrize("name", ["hg_value", "hg_cone_mean", "phase_value", "dipole_value", "random_direction", "direction_about", "lambert_lower_branch",
                                  "generalized_exp", "interpolate_loglog", "lnmean", "peel_taumax", "shifted_wavelength"])
def test_device_function(tiny, name):
    inputs = P.FUNCTIONS[name].inputs()
    assert 0 < len(inputs) <= 1 << 16
    got = tiny.device_function(name, inputs)
    bad = P.inadmissible(name, inputs, got)
    assert not bad, _show(bad)
    if name in ("hg_cone_mean", "phase_value"):
        assert np.isfinite(got).all() and (got > 0.).all()
    if name == "lambert_lower_branch":
        assert got[inputs[:, 0] == 0., 0] == -P.DBL_MAX and got[inputs[:, 0] == -P.INVERSE_E, 0] == -1.
    if name in ("random_direction", "direction_about"):
        # a unit vector, within the deviation of the restatement's own
        labels = P.branches(name, inputs)
        room = P.grouped_max(labels, P.norm_deviation(P.restated(name, inputs)))
        deviation = P.norm_deviation(got)
        for n, label in enumerate(labels):
            assert deviation[n] <= 4 * room[label] + 16 * math.ulp(1.), (name, tuple(inputs[n]), label, deviation[n], room[label])
    if name == "direction_about":
        # ... at the inclination asked for: k . k' = cos theta within what the restatement leaves (the pole branches ignore the tilt of k)
        room = P.grouped_max(labels, P.dot_deviation(inputs[:, :3], P.restated(name, inputs), inputs[:, 3]))
        deviation = P.dot_deviation(inputs[:, :3], got, inputs[:, 3])
        for n, label in enumerate(labels):
            assert deviation[n] <= 4 * room[label] + 16 * math.ulp(inputs[n, 3]), (tuple(inputs[n]), label, deviation[n], room[label])


def test_hg_cosine_and_the_direction_it_gives(tiny):
    """the HG cosine bit for bit, the flag of the isotropic branch, and every cosine -- those beyond +-1 included -- through directionAbout"""
    inputs = P.inputs_hg_cosine()
    got = tiny.device_function("hg_cosine", inputs)
    want = np.array([P.restate_hg_cosine(float(g), float(X)) for g, X in inputs])
    bad = P.inadmissible("hg_cosine", inputs, got[:, 0])
    assert not bad, _show(bad)
    assert np.array_equal(got[:, 1], want[:, 1]) and set(got[:, 1]) == {0., 1.}
    sampled = np.abs(inputs[:, 0]) >= 1e-6   # (what the scattering event hands on; below that it takes the isotropic branch)
    assert np.array_equal(got[:, 1] == 0., sampled)
    cosines = np.unique(got[sampled, 0])
    assert (np.abs(cosines) > 1.).any()
    tuples = P.inputs_direction_about(cosines=list(cosines))
    assert len(tuples) <= 1 << 16
    directions = tiny.device_function("direction_about", tuples)
    assert np.isfinite(directions).all()
    envelope = P.envelopes("direction_about", tuples)
    bad = P.inadmissible("direction_about", tuples, directions, envelope)
    assert not bad, _show(bad)
    labels = P.branches("direction_about", tuples)
    assert any(label.endswith("|beyond") for label in labels)
    room = P.grouped_max(labels, P.norm_deviation(P.restated("direction_about", tuples)))
    deviation = P.norm_deviation(directions)
    for n, label in enumerate(labels):
        assert deviation[n] <= 4 * room[label] + 16 * math.ulp(1.), (tuple(tuples[n]), label, deviation[n], room[label])


def test_locate(tiny):
    for key, nodes in P.locate_tables().items():
        x = P.locate_probes(nodes)
        for kind in ("locate", "locate_clip", "locate_basic"):
            assert np.array_equal(tiny.locate(kind, nodes, x), P.reference_locate(kind, nodes, x)), (key, kind)


def test_aids_refuse_what_they_cannot_run(tiny):
    """unknown function, too many tuples, a table of one node, no such instrument or source, a null buffer: an error, no launch"""
    two = np.array([[0.5, 0.5]])
    for call in (lambda: tiny.device_function(13, two), lambda: tiny.device_function(-1, two),
                 lambda: tiny.device_function("hg_value", two, n=(1 << 20) + 1), lambda: tiny.device_function("hg_value", two, n=-1),
                 lambda: tiny.device_function("hg_value", None, n=1),
                 lambda: tiny.locate("locate", [1.], [0.5]), lambda: tiny.locate("locate", None, [0.5], num_nodes=4), lambda: tiny.locate(3, [1., 2.], [0.5]),
                 lambda: tiny.detector(-1, [[0., 0., 0.]]), lambda: tiny.detector(16, [[0., 0., 0.]]), lambda: tiny.wavelength_bins(99, [1e-6]),
                 lambda: tiny.instrument_values(99), lambda: tiny.angular_probabilities(-1, [[0., 0., 1.]]), lambda: tiny.angular_probabilities(16, [[0., 0., 1.]]),
                 lambda: tiny.angular_probabilities(0, [[0., 0., 1.]])):   # (cfg1's source emits isotropically)
        with pytest.raises(RuntimeError, match="pmc error -1"):
            call()
    assert tiny.device_function("hg_value", np.empty((0, 2))).shape == (0, 1)
    assert np.array_equal(tiny.device_function("dipole_value", [[0.5]]), [[P.restate_dipole_value(0.5)]])   # (the context still works)


def _check_instrument(eng, index):
    """the pixel, the aperture flag and the wavelength bin of one instrument at its borders; returns its values"""
    I = eng.instrument_values(index)
    if I["include_ifu"]:
        r = P.frame_positions(I)
        i, j = P.pixel_coordinates(I, r)
        for coordinate, count in ((i, I["nxp"]), (j, I["nyp"])):
            for border in range(int(count) + 1):
                assert (coordinate == border - 1).any() and (coordinate == border).any(), (index, border)
        pixel, inside = eng.detector(index, r)
        assert np.array_equal(pixel, P.reference_pixel(I, r)), index
        assert np.array_equal(inside, P.reference_inside(I, r)), index
    if I["aperture_r2"] > 0.:
        r = P.aperture_positions(I)
        _, _, xpp, ypp = P.detector_plane(I, r)
        radius2 = xpp * xpp + ypp * ypp
        assert (radius2 > I["aperture_r2"]).any() and (radius2 < I["aperture_r2"]).any()
        _, inside = eng.detector(index, r)
        assert np.array_equal(inside, P.reference_inside(I, r)) and set(inside) == {0, 1}, index
    lam = P.bin_wavelengths(I)
    seen = lam * I["zp1"]
    for b in I["border"]:
        assert (seen < b).any() and (seen >= b).any()
    assert np.array_equal(eng.wavelength_bins(index, lam), P.reference_bin(I, lam)), index
    return I


def test_frames_and_bins_of_a_rotated_offset_frame_at_redshift():
    """cfg3z: six instruments at redshift 0.5, among them a rolled, offset frame of 16 x 12 pixels"""
    sim, eng = _context("cfg3z.ski")
    values = [_check_instrument(eng, index) for index in range(6)]
    tilted = values[1]
    assert (tilted["nxp"], tilted["nyp"]) == (16, 12) and tilted["sinomega"] != 0. and tilted["xpmin"] != -tilted["nxp"] * tilted["xpsiz"] / 2.
    assert tilted["xpsiz"] != tilted["ypsiz"] and len(tilted["border"]) >= 2
    # (an instrument without a distance of its own is in the observer frame, one with a distance sees the rest frame)
    assert {v["zp1"] for v in values} == {1., 1.5}
    with pytest.raises(RuntimeError, match="pmc error -1"):
        eng.detector(6, [[0., 0., 0.]])
    del eng, sim


def test_aperture_of_an_sed_instrument():
    """cfg1sed: an SEDInstrument with an aperture of 0.4 pc next to one without"""
    sim, eng = _context("cfg1sed.ski")
    count = 0
    while count < 16:
        try:
            eng.instrument_values(count)
        except RuntimeError:
            break
        count += 1
    values = [_check_instrument(eng, index) for index in range(count)]
    pc = 3.08567758e16   # (the host layer's parsec: skirt9_amd/host/units.hpp)
    radii = sorted(math.sqrt(v["aperture_r2"]) / pc for v in values)
    assert count >= 2 and radii[0] == 0. and abs(radii[-1] - 0.4) < 1e-12, radii
    del eng, sim


@pytest.mark.parametrize("scene, kind", [("cfg1laser.ski", P.ANGULAR_LASER), ("cfg1con.ski", P.ANGULAR_CONICAL), ("cfg1netzer.ski", P.ANGULAR_NETZER)])
def test_angular_probability(scene, kind):
    sim, eng = _context(scene)
    _, got_kind, axis, cos_delta = eng.angular_probabilities(0, np.empty((0, 3)))
    assert got_kind == kind and abs(np.linalg.norm(axis) - 1.) < 1e-15
    k = P.angular_directions(kind, axis, cos_delta)
    p, _, _, _ = eng.angular_probabilities(0, k)
    want = np.array([P.restate_angular_probability(kind, axis, cos_delta, row) for row in k])
    assert np.array_equal(P.bits(p), P.bits(want)), (k[P.bits(p) != P.bits(want)][:3], p[P.bits(p) != P.bits(want)][:3])
    if kind == P.ANGULAR_LASER:
        assert set(p) == {0., math.inf}
    elif kind == P.ANGULAR_CONICAL:
        assert set(p) == {0., 1.0 / (1.0 - cos_delta)}
    with pytest.raises(RuntimeError, match="pmc error -1"):
        eng.angular_probabilities(1, k)
    del eng, sim
