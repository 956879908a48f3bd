"""Moving sources on the GPU (run with `pytest -m gpu`): the Doppler shift of what a source with a bulk velocity emits
(skirt9_amd/csrc/pmc_launch.inc launchHistory, pmc_cycle.inc startCycleWalks, pmc_transition.inc onCycleDone: the kinematic flavours of the launch, cycle start and
transition kernels).

The CPU oracle (oracle/life_cycle.cpp) has no Doppler shift.  It is used through an identity: a source whose velocity v is the same for all
its packets shifts every emission peel-off packet towards observer g by ONE factor f_g = 1 - k_g.v/c.  The transparent flux of the moving
scene in instrument g is then that of the same histories in a STATIC twin scene whose instrument g has its wavelength grid divided by f_g,
times 1/f_g (the detected luminosity is W / lambda); with gray dust the same holds for the direct flux.  The unmodified reference confirms
the identity to 1e-10 (moving against static twin, single thread).  Where the dust is not gray the cross section of the direct path is
pinned against the dust table itself; the velocity fields against their closed forms; and the whole -- rotation curve, scattered light --
statistically against files of the unmodified reference."""

import os
import re
import subprocess

import numpy as np
import pytest

import kinematics_checks as K
import oracle_lib as O
from conftest import ROOT, golden, ski
from electron_checks import meets_stated_criteria
from skirt9_amd.host import Simulation, scene_head
from test_gpu_electrons import PRIMARY_DIRECT, TRANSPARENT, _component_blocks, _num_instruments, _with_blocks_of
from test_gpu_parity import _compare_frames, _engine

pytestmark = pytest.mark.gpu

C_LIGHT = 2.99792458e8
PC = 3.08567758e16   # (the parsec of the host layer's unit table, as the reference has it)
N = 20000
SEED = 314159

# the observers of the instruments i0 .. i4 of cfg1kin, cfg3kinbox and cfg5kin: (inclination, azimuth) in degrees; i2 shares the observer of i1
OBSERVERS = [(0., 0.), (90., 0.), (90., 0.), (90., 180.), (55., 70.)]


def _kobs(inclination, azimuth):
    i, a = np.radians(inclination), np.radians(azimuth)
    return np.array([np.sin(i) * np.cos(a), np.sin(i) * np.sin(a), np.cos(i)])


def _factors(velocity):
    """f_g = 1 - k_g.v/c of every instrument for a source with the velocity v (m/s)"""
    return [1. - float(np.dot(_kobs(*o), velocity)) / C_LIGHT for o in OBSERVERS]


def _lin_borders(lo, hi, n):
    """bin borders of a LinWavelengthGrid: midpoints of its n wavelengths, the outer ones mirrored (DisjointWavelengthGrid.cpp:22-60)"""
    lam = np.linspace(lo, hi, n)
    return np.concatenate([[(3. * lam[0] - lam[1]) / 2.], (lam[:-1] + lam[1:]) / 2., [(3. * lam[-1] - lam[-2]) / 2.]])


def _static_twin(text, factors):
    """the ski text of the static twin: no velocity, and the wavelength grid of instrument g divided by f_g"""
    text, moved = re.subn(r'velocity(X|Y|Z|Magnitude)="[^"]*"', lambda m: 'velocity%s="0 km/s"' % m.group(1), text)
    assert moved >= 1
    head, tail = text.split("<instruments", 1)
    grids = iter(factors)

    def scaled(m):
        f = next(grids)
        return 'minWavelength="%r micron" maxWavelength="%r micron"' % (float(m.group(1)) / f, float(m.group(2)) / f)

    tail, count = re.subn(r'minWavelength="([0-9.e+-]+) micron" maxWavelength="([0-9.e+-]+) micron"', scaled, tail)
    assert count == len(factors)
    return head + "<instruments" + tail


def _variant(text, forced=True, explicit_absorption=False):
    old = 'explicitAbsorption="false" forceScattering="true"'
    assert old in text
    return text.replace(old, 'explicitAbsorption="%s" forceScattering="%s"' % ("true" if explicit_absorption else "false", "true" if forced else "false"))


VELOCITY = {"cfg1kin": np.array([1500e3, -900e3, 2100e3]), "cfg5kin": np.array([1500e3, -900e3, 2100e3]),
            "cfg3kinbox": 1800e3 * np.array([1., -2., 0.5]) / np.linalg.norm([1., -2., 0.5])}

_runs = {}


def _moving_and_twin(tmp_path_factory, name, forced, ea):
    """one engine run of the moving scene, one oracle run (Philox streams) of its static twin; shared, and nobody changes the arrays"""
    key = (name, forced, ea)
    if key not in _runs:
        text = _variant(open(ski(name + ".ski")).read(), forced, ea)
        factors = _factors(VELOCITY[name])
        d = tmp_path_factory.mktemp("kin")
        (d / "moving.ski").write_text(text)
        (d / "twin.ski").write_text(_static_twin(text, factors))
        sim = Simulation(str(d / "moving.ski"), num_packets=N).setup()
        assert any(v["kind"] for v in sim.source_velocities)
        eng = _engine(sim)
        eng.run_primary(0, N, SEED)
        gpu = eng.download()
        counters = eng.counters()
        eng.close()
        twin = Simulation(str(d / "twin.ski"), num_packets=N).setup()
        assert not any(v["kind"] for v in twin.source_velocities) and twin.frame_size == sim.frame_size
        ref, _ = O.run_primary(twin, 0, N, O.RNG_PHILOX, seed=SEED)
        gpu.setflags(write=False)
        ref.setflags(write=False)
        _runs[key] = (sim, gpu, ref, counters, factors)
    return _runs[key]


CASES = [("cfg1kin", True, False), ("cfg1kin", False, True), ("cfg3kinbox", True, False), ("cfg3kinbox", False, False), ("cfg5kin", True, False)]


@pytest.mark.parametrize("name,forced,ea", CASES)
def test_emission_against_the_oracle_on_the_static_twin(tmp_path_factory, name, forced, ea):
    """Transparent and PrimaryDirect flux of every instrument, SED and IFU, of 2e4 histories: the engine on the moving scene against the
    oracle on the static twin times 1/f_g, under _compare_frames' own tolerances.  Cartesian, octree and Voronoi grid; forced and
    non-forced scattering, explicit absorption; three distinct observers, one shared, one in the observer frame of the model's redshift.
    Unscaled -- the twin's frames as they are -- the comparison fails."""
    sim, gpu, ref, counters, factors = _moving_and_twin(tmp_path_factory, name, forced, ea)
    assert counters["histories"] == N and counters["stat_overflows"] == 0 and counters["scatterings"] > 0
    assert _num_instruments(sim) == len(factors) and len(set(round(f, 12) for f in factors)) == 4
    got, want, blocks = ref.copy(), ref.copy(), []
    for inst, f in enumerate(factors):
        mine = _component_blocks(sim, inst, TRANSPARENT) + _component_blocks(sim, inst, PRIMARY_DIRECT)
        assert all(np.count_nonzero(ref[at:at + count]) > 0 for at, count in mine)
        got = _with_blocks_of(got, gpu, mine)
        want = _with_blocks_of(want, ref, mine, 1. / f)
        blocks += mine
    _compare_frames(sim, got, want, N)
    with pytest.raises(AssertionError):
        _compare_frames(sim, got, ref, N)


@pytest.mark.parametrize("groups", ["1", "3"])
def test_reused_slots(tmp_path_factory, monkeypatch, groups):
    """cfg1kin in 4096 slots -- every slot takes up five histories, and its per-observer values with them -- in one slot group and in three:
    the counted work of the default run exactly, its frames to _compare_frames' tolerances"""
    sim, gpu, _, counters, _ = _moving_and_twin(tmp_path_factory, "cfg1kin", True, False)
    monkeypatch.setenv("PMC_NUM_GROUPS", groups)   # (read by pmc_create)
    eng = _engine(sim)
    eng.set_num_slots(4096)
    eng.run_primary(0, N, SEED)
    again = eng.download()
    c = eng.counters()
    assert eng.last_timing()["generations"] >= N / 4096
    eng.close()
    for key in ("histories", "paths", "cell_visits", "scatterings", "stat_overflows"):
        assert c[key] == counters[key], key
    # _compare_frames also holds the frames to an invariant of a scene at rest: a history reaches ONE wavelength bin of an SED, so the
    # counts of histories per bin (the w^0 row of instrument 0's statistics) sum to n.  Here a history reaches up to two -- the bin of
    # its emission peel-off packet and the bin of the packet itself, for its scattered light (FluxRecorder sums a history's
    # contributions per bin) -- so that row is compared here, exactly, and goes to _compare_frames as a row that sums to N in both runs
    lay = sim.layout(0)
    row = slice(lay.wsed_offset, lay.wsed_offset + lay.num_lambda)
    assert lay.wsed_offset >= 0 and np.array_equal(again[row], gpu[row]) and N < gpu[row].sum() <= 2 * N
    a, b = again.copy(), gpu.copy()
    a[row] = b[row] = 0.
    a[row.start] = b[row.start] = N
    _compare_frames(sim, a, b, N)


def test_cross_section_at_the_observers_wavelength():
    """cfg1kinsteep: a moving point source in dust whose cross section falls steeply with wavelength; the instruments have narrow bins, most of
    them inside one bin of the dust table (which holds the instruments' wavelengths).  All packets start at one point, so the
    direct path towards observer g has ONE column density N_g (trace_ray times the cell densities), and every packet in a wavelength bin of
    instrument g that lies inside one bin il of the dust table saw exp(-sigma_ext[il] N_g): PrimaryDirect / Transparent of that bin, to 1e-9
    (the project's tolerance for sums).  The cross sections at the unshifted wavelength lambda0 and at the wavelength of a packet launched
    away from the observer give values that are off by more than 1e-4: the three wavelengths are told apart."""
    n = N
    sim = Simulation(ski("cfg1kinsteep.ski"), num_packets=n).setup()
    eng = _engine(sim)
    eng.run_primary(0, n, SEED)
    gpu = eng.download()
    medium = scene_head(sim).medium
    nl = medium.num_lambda
    border = np.ctypeslib.as_array(medium.lambda_border, shape=(nl,))
    sigma = np.ctypeslib.as_array(medium.sigma_ext, shape=(nl,))
    density = np.ctypeslib.as_array(medium.number_density, shape=(scene_head(sim).grid.num_cells,))

    def dust_bin(lam):   # DustMix::indexForLambda: NR::locateClip on the borders
        return int(np.clip(np.searchsorted(border, lam, side="right") - 1, 0, nl - 2))

    position = np.array([0.2, -0.1, 0.3]) * PC
    velocity = np.array([1500e3, -900e3, 2100e3])
    text = open(ski("cfg1kinsteep.ski")).read().split("<instruments", 1)[1]
    lists = re.findall(r'<ListWavelengthGrid wavelengths="([^"]*)" relativeHalfWidth="2e-5"', text)
    assert len(lists) == len(OBSERVERS)
    checked = 0
    for inst, (obs, f) in enumerate(zip(OBSERVERS, _factors(velocity))):
        k = _kobs(*obs)
        m, ds = eng.trace_ray(position, k)
        column = float(np.sum(density[m[m >= 0]] * ds[m >= 0]))
        assert column > 0
        li = sim.layout(inst)
        # the instrument's bins: relative half width 2e-5 around its listed wavelengths (DisjointWavelengthGrid::setWavelengthBins), in the
        # observer frame of i4; the packets in them have the rest wavelengths bin / (1 + z)
        centres = np.array([float(w.split()[0]) * 1e-6 for w in lists[inst].split(",")])
        bins = len(centres)
        assert bins == li.num_lambda
        zp1 = 1.02 if inst == 4 else 1.
        transparent = gpu[li.sed_offset + TRANSPARENT * bins:li.sed_offset + (TRANSPARENT + 1) * bins]
        direct = gpu[li.sed_offset + PRIMARY_DIRECT * bins:li.sed_offset + (PRIMARY_DIRECT + 1) * bins]
        for ell in np.nonzero(transparent)[0]:
            left, right = centres[ell] * (1. - 2.1e-5) / zp1, centres[ell] * (1. + 2.1e-5) / zp1      # the bin with a margin for its rounded borders
            il = dust_bin(left)
            if il != dust_bin(right):
                continue
            want = np.exp(-sigma[il] * column)
            got = direct[ell] / transparent[ell]
            assert abs(got - want) <= 1e-9 * want, (inst, ell, got, want)
            centre = centres[ell] / zp1
            for other in (centre / f, centre / f * (2. - f)):      # lambda0; a packet launched away from the observer
                assert abs(np.exp(-sigma[dust_bin(other)] * column) - want) > 1e-4 * want, (inst, ell, other)
            checked += 1
    eng.close()
    assert checked >= 40, checked


def _closed_form(kind, magnitude, offset, unity_radius, exponent, r):
    x = r - np.asarray(offset)
    u = x.copy() if kind == "radial" else np.stack([-x[:, 1], x[:, 0], np.zeros(len(x))], axis=1)
    norm = np.sqrt((u ** 2).sum(axis=1))
    v = np.ones(len(x))
    if unity_radius > 0:
        inside = (norm < unity_radius) if exponent > 0 else (norm > unity_radius)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(inside & (exponent != 0), (norm / unity_radius) ** exponent, 1.)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = magnitude * v[:, None] * u / norm[:, None]
    out[norm == 0] = 0.
    return out


FIELDS = [("uni", '<UnidirectionalVectorField fieldX="1" fieldY="-2" fieldZ="0.5"/>', None),
          ("radial", '<RadialVectorField unityRadius="1500 pc" exponent="0.5"/>', ("radial", (0., 0., 0.), 1500 * PC, 0.5)),
          ("radialdefault", '<RadialVectorField/>', ("radial", (0., 0., 0.), 0., 1.)),
          ("cyl", '<CylindricalVectorField unityRadius="2000 pc" exponent="1"/>', ("cyl", (0., 0., 0.), 2000 * PC, 1.)),
          ("cylneg", '<CylindricalVectorField unityRadius="2000 pc" exponent="-0.5"/>', ("cyl", (0., 0., 0.), 2000 * PC, -0.5)),
          ("offset", '<OffsetVectorFieldDecorator offsetX="300 pc" offsetY="-200 pc" offsetZ="100 pc"><vectorField type="VectorField">'
                     '<CylindricalVectorField unityRadius="2000 pc" exponent="1"/></vectorField></OffsetVectorFieldDecorator>',
           ("cyl", (300 * PC, -200 * PC, 100 * PC), 2000 * PC, 1.))]


@pytest.mark.parametrize("label,field,form", FIELDS, ids=[f[0] for f in FIELDS])
def test_velocity_fields_against_closed_forms(tmp_path, label, field, form):
    """pmc_tune_source_velocities: the launch kernel's velocity function at 2^12 positions -- random ones, the origin, points on the z-axis
    and on the field's own axis -- against numpy's evaluation of UnidirectionalVectorField, RadialVectorField.cpp:17-35 and
    CylindricalVectorField.cpp:17-36 (default: magnitude 1 everywhere; the null vector at the origin resp. on the axis), alone and inside an
    OffsetVectorFieldDecorator.  1e-14 times the magnitude: a handful of operations and one pow, each good to a few ulp, with a tenfold margin."""
    magnitude = 1800e3
    text = open(ski("cfg3kinbox.ski")).read()
    old = '<UnidirectionalVectorField fieldX="1" fieldY="-2" fieldZ="0.5"/>'
    assert old in text
    (tmp_path / "f.ski").write_text(text.replace(old, field))
    sim = Simulation(str(tmp_path / "f.ski"), num_packets=100).setup()
    eng = _engine(sim)
    rng = np.random.default_rng(5)
    r = (rng.random((1 << 12, 3)) - 0.5) * 2 * 5000 * PC
    centre = np.asarray(form[1]) if form else np.zeros(3)
    r[0] = 0.
    r[1] = centre
    r[2:10, :2] = 0.                       # on the z-axis
    r[10:20, :2] = centre[:2]              # on the field's axis
    r[20:30] *= 1e-3                       # well inside the unity radius
    got = eng.source_velocities(0, r)
    eng.close()
    if form is None:
        want = np.tile(magnitude * np.array([1., -2., 0.5]) / np.sqrt(1. + 4. + 0.25), (len(r), 1))
    else:
        want = _closed_form(form[0], magnitude, form[1], form[2], form[3], r)
        assert np.all(want[1] == 0.) and (form[0] == "radial" or np.all(want[10:20] == 0.))
    assert np.abs(got - want).max() <= 1e-14 * magnitude, float(np.abs(got - want).max())
    assert np.abs(want).max() > 0.5 * magnitude


def test_command_line_run_writes_shifted_lines(tmp_path):
    """skirt_mi355x on cfg1kin: the transparent line of every instrument's SED file peaks in the bin of 0.55 micron times f_g (times 1 + z in the
    observer frame of i4), not in the bin of 0.55 micron"""
    exe = os.path.join(ROOT, "skirt9_amd", "lib", "skirt_mi355x")
    subprocess.run([exe, "-o", str(tmp_path), "-n", str(N), ski("cfg1kin.ski")], check=True, stdout=subprocess.DEVNULL)
    moved = 0
    for inst, f in enumerate(_factors(VELOCITY["cfg1kin"])):
        table = np.loadtxt(str(tmp_path / ("cfg1kin_i%d_sed.dat" % inst)))
        wavelength, transparent = table[:, 0], table[:, 2]
        zp1 = 1.02 if inst == 4 else 1.
        peak = int(np.argmax(transparent))
        assert peak == int(np.argmin(np.abs(wavelength - 0.55 * f * zp1))), (inst, wavelength[peak], 0.55 * f * zp1)
        moved += peak != int(np.argmin(np.abs(wavelength - 0.55 * zp1)))
    assert moved >= 4


def test_rotating_disk_within_noise_of_the_reference(tmp_path):
    """cfg3kin, 10^6 packets: an exponential disk of stars that rotates at 2400 km/s (rigidly inside 2000 pc) and a point source that moves
    along z, through dust that is steep across the widened wavelength range, against what the UNMODIFIED reference wrote for the scene
    with its own generator (tests/golden/cfg3kin_rebinned.npz, made by tests/golden/make_golden_kinematics.py: total flux and statistics
    cubes summed over 8 x 8 blocks per wavelength bin).  Every block of every wavelength bin with 30 contributions in both runs -- direct
    and scattered light -- under the criteria of electron_checks.meets_stated_criteria: reduced chi^2 in [0.85, 1.2], no block beyond 5.5
    sigma, integrated flux within 3 sigma, more than 500 blocks.  (Two runs of the reference with different seeds give chi^2 1.048, 3.35
    sigma, 0.29 sigma over 792 blocks; the scene at rest gives chi^2 1724: see the generator.)  And the sign: per block column of the
    edge-on frame the mean velocity runs monotonically from approaching to receding across the disk and stays within +-V (the reference:
    -2144 ... +2150 km/s); the disk seen face-on shows none."""
    n = 1000000
    instruments = ("edge", "face")
    sim = Simulation(ski("cfg3kin.ski"), num_packets=n).setup()
    eng = _engine(sim)
    eng.run_primary(0, n, 20261017)
    c = eng.counters()
    assert c["histories"] == n and c["stat_overflows"] == 0
    sim.write(eng.download(), str(tmp_path))
    eng.close()
    gpu = K.rebinned_cubes(str(tmp_path), "cfg3kin", instruments)
    gold = np.load(golden("cfg3kin_rebinned.npz"))
    chi2, zmax, flux_sigmas, blocks = K.all_light(gpu, n, gold, n, instruments)
    print(f"cfg3kin: reduced chi^2 {chi2:.4f} over {blocks} blocks, largest |z| {zmax:.2f}, integrated flux {flux_sigmas:.2f} sigma")
    velocity = K.column_velocities(gpu["edge_total"], gold["wavelengths"], 0.55e-6)
    print("cfg3kin: edge-on mean velocity per block column (km/s):", np.round(velocity / 1e3, 1))
    assert blocks > 500
    assert 0.85 <= chi2 <= 1.2, chi2
    assert zmax < 5.5, zmax
    assert flux_sigmas <= 3, flux_sigmas
    assert meets_stated_criteria(chi2, zmax, flux_sigmas, blocks)
    assert np.all(np.diff(velocity) > 0) and velocity[0] < -1500e3 and velocity[-1] > 1500e3
    assert np.all(np.abs(velocity) < 2400e3)
    face = K.column_velocities(gpu["face_total"], gold["wavelengths"], 0.55e-6)
    assert np.all(np.abs(face[[0, 1, 2, 5, 6, 7]]) < 30e3), face     # (the central columns hold the point source, which approaches at 1200 km/s)
