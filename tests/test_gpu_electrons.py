"""Electron media on the GPU (run with `pytest -m gpu`): Thomson scattering with the dipole phase function in the transition kernel
(skirt9_amd/csrc/pmc_phase.inc PhaseDipole), alone and next to dust components.

The CPU oracle (oracle/life_cycle.cpp) has no dipole: it reads an electron component as an isotropic scatterer with the same opacities.
So the oracle pins everything the phase function cannot touch, and -- where all first scatterings share one incoming direction -- the
peel-off value itself, as a known factor on the oracle's frames; the sampler is checked on its own against the closed form, and the
whole against the files of the UNMODIFIED reference, statistically."""

import numpy as np
import pytest

import electron_checks as E
import oracle_lib as O
from conftest import golden, ski
from skirt9_amd.host import Simulation
from test_gpu_parity import _compare_frames, _engine

pytestmark = pytest.mark.gpu

TRANSPARENT, PRIMARY_DIRECT, LEVEL_1 = 0, 1, 3      # components of an instrument with recordComponents (include/pmc.h pmc_frame_layout)


def _component_blocks(sim, instrument, component):
    """(offset, count) of one flux component of an instrument in the frame buffer: SED and IFU"""
    li = sim.layout(instrument)
    assert component < li.num_components
    blocks = []
    if li.sed_offset >= 0:
        blocks.append((li.sed_offset + component * li.num_lambda, li.num_lambda))
    if li.ifu_offset >= 0:
        blocks.append((li.ifu_offset + component * li.npix * li.num_lambda, li.npix * li.num_lambda))
    return blocks


def _with_blocks_of(base, other, blocks, scale=1.):
    """a copy of `base` in which the listed blocks hold `other`'s values (times scale): _compare_frames then compares those blocks alone,
    under its own tolerances -- everywhere else it sees equal arrays"""
    out = base.copy()
    for at, count in blocks:
        out[at:at + count] = other[at:at + count] * scale
    return out


def _num_instruments(sim):
    n = 0
    try:
        while True:
            sim.layout(n)
            n += 1
    except IndexError:
        return n


_runs = {}


def _engine_and_oracle(name, n, seed=12345):
    """one engine run and one oracle run (Philox streams) of a scene, shared by the tests that need them; nobody changes the arrays"""
    if name not in _runs:
        sim = Simulation(ski(name), num_packets=n).setup()
        eng = _engine(sim)
        eng.run_primary(0, n, seed)
        gpu = eng.download()
        counters = eng.counters()
        eng.close()
        ref, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=seed)
        gpu.setflags(write=False)
        ref.setflags(write=False)
        _runs[name] = (sim, gpu, ref, counters)
    return _runs[name]


SCENES = [("cfg1elec.ski", 20000), ("cfg1eleclaser.ski", 20000), ("cfg1elecnf.ski", 50000), ("cfg2agnelec.ski", 20000), ("cfg2agnelecea.ski", 20000),
          ("cfg5elec.ski", 20000)]


@pytest.mark.parametrize("name,n", SCENES)
def test_what_the_phase_function_cannot_touch(name, n):
    """Transparent and PrimaryDirect flux of every instrument that records components, SED and IFU, against the oracle: the emission
    peel-off of the same histories through the same opacities -- normalization of the electron medium, its cross sections, the
    bookkeeping of several components, the direct path.  Forced and non-forced scattering, explicit absorption, all three grids; every
    history is counted."""
    sim, gpu, ref, counters = _engine_and_oracle(name, n)
    assert counters["histories"] == n and counters["stat_overflows"] == 0 and counters["scatterings"] > 0
    blocks = []
    for inst in range(_num_instruments(sim)):
        if sim.layout(inst).num_components >= 3:
            blocks += _component_blocks(sim, inst, TRANSPARENT) + _component_blocks(sim, inst, PRIMARY_DIRECT)
    # (the laser of cfg1eleclaser points away from every observer: there both components are zero, in the engine as in the oracle)
    assert blocks and ("laser" in name or sum(np.count_nonzero(ref[at:at + count]) for at, count in blocks) > 0)
    _compare_frames(sim, _with_blocks_of(ref, gpu, blocks), ref, n)


def test_peel_off_value_of_the_dipole():
    """cfg1eleclaser: the source emits along +z, so before its first scattering every history is the same in the engine and in the oracle,
    and every first scattering has the incoming direction +z.  The oracle weighs the peel-off packet of a first scattering with the isotropic
    phase function (1), the engine with the dipole's 0.75 (1 + cos^2 i) towards the observer at inclination i: the level-1 scattered flux
    of the engine is the oracle's times 1.3125, 0.75 and 1.3125 at 30, 90 and 150 degrees, pixel by pixel.  (On the commit before this one
    the scene does not load: ElectronMix was refused.)"""
    n = 20000
    sim, gpu, ref, _ = _engine_and_oracle("cfg1eleclaser.ski", n)
    factors = [0.75 * (1. + np.cos(np.radians(i)) ** 2) for i in (30., 90., 150.)]
    assert np.allclose(factors, [1.3125, 0.75, 1.3125], rtol=1e-15)
    for inst, factor in enumerate(factors):
        blocks = _component_blocks(sim, inst, LEVEL_1)
        assert all(np.count_nonzero(ref[at:at + count]) > 0 for at, count in blocks)
        _compare_frames(sim, _with_blocks_of(ref, gpu, blocks), _with_blocks_of(ref, ref, blocks, factor), n)
    # the comparison does compare: without the factor the arrays at 90 degrees disagree
    blocks = _component_blocks(sim, 1, LEVEL_1)
    with pytest.raises(AssertionError):
        _compare_frames(sim, _with_blocks_of(ref, gpu, blocks), ref, n)


def test_dipole_sampler():
    """pmc_tune_dipole_cosines: the device function of the scattering step, over 2^16 midpoints of [0, 1], against numpy's evaluation of the
    closed form p - 1/p, p = cbrt(4X - 2 + sqrt(16X(X - 1) + 5)) (DipolePhaseFunction.cpp:54-59).  1e-14 absolute: each of the few
    operations on values <= 5 is good to a few ulp (2.2e-16 relative), which leaves a tenfold margin.  Midpoint quadrature of the moments:
    <cos> = 0, <cos^2> = 2/5 (an isotropic scatterer has 1/3)."""
    sim = Simulation(ski("cfg1elec.ski"), num_packets=100).setup()
    eng = _engine(sim)
    N = 1 << 16
    X = (np.arange(N) + 0.5) / N
    got = eng.dipole_cosines(X)
    p = np.cbrt(4. * X - 2. + np.sqrt(16. * X * (X - 1.) + 5.))
    want = p - 1. / p
    assert np.abs(got - want).max() <= 1e-14, float(np.abs(got - want).max())
    assert got.min() >= -1. and got.max() <= 1.
    assert np.all(np.diff(got) > 0)
    assert abs(got.mean()) <= 1e-6, float(got.mean())
    assert abs((got ** 2).mean() - 0.4) <= 1e-6, float((got ** 2).mean())


@pytest.mark.parametrize("name,instruments", [("cfg1elec", ("i30", "i90", "i150")), ("cfg2agnelec", ("i0", "i1"))])
def test_scattered_light_within_noise_of_the_reference(name, instruments, tmp_path):
    """10^6 packets on the GPU against what the UNMODIFIED reference wrote for the scene with its own generator
    (tests/golden/<name>_rebinned.npz, made by tests/golden/make_golden_electrons.py: flux and statistics frames summed over 8 x 8 blocks),
    by the method of test_fits_cube_within_noise_of_the_reference on the blocks the direct light does not reach: scattered light alone.
    That test's criteria: reduced chi^2 in [0.85, 1.2], no block beyond 5.5 sigma, integrated flux within 3 sigma.  (Two runs of the
    reference with different seeds meet them; an isotropic scatterer in the electrons' place gives chi^2 of 8 and more: see the generator.)"""
    n = 1000000
    sim = Simulation(ski(name + ".ski"), num_packets=n).setup()
    eng = _engine(sim)
    eng.run_primary(0, n, 20260929)
    assert eng.counters()["histories"] == n
    sim.write(eng.download(), str(tmp_path))
    gpu = E.rebinned_files(str(tmp_path), name, instruments)
    gold = np.load(golden(name + "_rebinned.npz"))
    chi2, zmax, flux_sigmas, blocks = E.scattered_light(gpu, n, gold, n, instruments)
    print(f"{name}: reduced chi^2 {chi2:.4f} over {blocks} blocks, largest |z| {zmax:.2f}, integrated flux {flux_sigmas:.2f} sigma")
    assert blocks > 500
    assert 0.85 <= chi2 <= 1.2, chi2
    assert zmax < 5.5, zmax
    assert flux_sigmas <= 3, flux_sigmas


def _radiation_field_variant(tmp_path, one_path_only):
    """cfg2agnelecea (octree, electrons + dust, explicit absorption) with the radiation field stored; one_path_only: every history ends
    after its first forced path -- no path-length bias, and minWeightReduction 1: the weight after the first interaction,
    W (1 - e^-tau_path) e^-tau_abs, is below the launch weight"""
    text = open(ski("cfg2agnelecea.ski")).read()
    assert 'storeRadiationField="false"' in text and 'minWeightReduction="1e4"' in text and 'pathLengthBias="0.5"' in text
    text = text.replace('storeRadiationField="false"', 'storeRadiationField="true"')
    if one_path_only:
        text = text.replace('minWeightReduction="1e4"', 'minWeightReduction="1"').replace('pathLengthBias="0.5"', 'pathLengthBias="0"')
    p = tmp_path / ("cfg2agnelecearf1.ski" if one_path_only else "cfg2agnelecearf.ski")
    p.write_text(text)
    return str(p)


def test_radiation_field_with_electrons(tmp_path):
    """storeRadiationField next to an electron component.  The field depends on paths, and the paths of the engine and of the (isotropic)
    oracle are the same only until the first scattering: with histories that end after their first forced path the table equals the
    oracle's under the tolerance of test_radiation_field_matches_oracle, and so do the frames; with the usual histories the run completes."""
    n = 20000
    sim = Simulation(_radiation_field_variant(tmp_path, True), num_packets=n).setup()
    eng = _engine(sim)
    assert eng.radiation_field_size == sim.radiation_field_size > 0
    eng.run_primary(0, n, 5)
    gpu_frames, gpu_rf = eng.download(), eng.download_radiation_field()
    c = eng.counters()
    assert c["histories"] == n and c["scatterings"] == 0
    ref_frames, ref_rf, _ = O.run_primary_rf(sim, 0, n, O.RNG_PHILOX, seed=5)
    assert ref_rf.sum() > 0
    assert abs(gpu_rf.sum() - ref_rf.sum()) <= 1e-9 * ref_rf.sum()
    assert np.array_equal(gpu_rf > 0, ref_rf > 0)
    bad = np.abs(gpu_rf - ref_rf) > 1e-6 * np.abs(ref_rf) + 1e-13 * ref_rf.max()
    assert bad.sum() == 0, int(bad.sum())
    _compare_frames(sim, gpu_frames, ref_frames, n)
    eng.close()
    # the usual histories
    sim = Simulation(_radiation_field_variant(tmp_path, False), num_packets=n).setup()
    eng = _engine(sim)
    eng.run_primary(0, n, 5)
    c = eng.counters()
    assert c["histories"] == n and c["scatterings"] > n
    rf = eng.download_radiation_field()
    assert np.all(np.isfinite(rf)) and rf.sum() > gpu_rf.sum()


def test_scene_file_runs_with_its_extension(tmp_path):
    """a scene loaded from a file runs the dipole as the live scene does (same histories, same kernels: equal to summation order)"""
    from skirt9_amd.host import SceneFile
    n = 5000
    sim, gpu, _, _ = _engine_and_oracle("cfg1eleclaser.ski", 20000)
    path = str(tmp_path / "scene.bin")
    sim.save_scene(path)
    loaded = SceneFile(path)
    a, b = _engine(sim), _engine(loaded)
    a.run_primary(0, n, 9)
    b.run_primary(0, n, 9)
    x, y = a.download(), b.download()
    assert x.sum() > 0 and np.allclose(x, y, rtol=1e-10, atol=1e-13 * np.abs(x).max())
    # ... and not as Henyey-Greenstein: without the extension the same scene gives other level-1 frames
    from skirt9_amd.engine import Engine
    plain = Engine(int(loaded.scene), 0)
    plain.run_primary(0, n, 9)
    z = plain.download()
    at, count = _component_blocks(sim, 1, LEVEL_1)[-1]
    assert np.allclose(x[at:at + count], 0.75 * z[at:at + count], rtol=1e-6, atol=1e-12 * np.abs(z[at:at + count]).max())
