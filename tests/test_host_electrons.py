"""Electron media in the host model layer (ElectronMix: Thomson scattering with the dipole phase function): the cell densities and
cross sections against the reference's cell dump, the refused variants, and the scene file with its extension."""
import re
import struct

import numpy as np
import pytest

import oracle_lib as O
from conftest import golden, ski
from skirt9_amd.host import SceneFile, Simulation, scene_head

PMC_PHASE_HG, PMC_PHASE_DIPOLE = 0, 1
SIGMA_THOMSON = 6.6524587158e-29


@pytest.mark.parametrize("name,cells", [("cfg1elec", 32768), ("cfg2agnelec", 22667)])
def test_electron_cell_densities_bit_exact(name, cells):
    """component 0 of both scenes is the electron medium (optical depth / number normalization); on the octree of cfg2agnelec the cell
    count also pins the tree policy, which refines on the dust of the torus AND on the electron number (DensityTreePolicy.cpp:87-94, 211-216)"""
    sim = Simulation(ski(name + ".ski")).setup()
    head = scene_head(sim)
    assert head.grid.num_cells == cells
    gold = np.load(golden(name + "_cells.npz"))
    assert gold["density"].size == cells and gold["density"].max() > 0
    dens = np.ctypeslib.as_array(head.medium.number_density, shape=(cells,))
    assert np.array_equal(dens.view(np.uint64), gold["density"].view(np.uint64))
    m = head.medium
    lam = np.ctypeslib.as_array(m.lambda_border, shape=(m.num_lambda,))
    # borders that span the simulation's wavelength range: every wavelength of the simulation finds the one cross section
    assert lam[0] <= 0.55e-6 / 1.01 and lam[-1] >= 0.55e-6
    idx = max(0, np.searchsorted(lam, 0.55e-6, side="right") - 1)
    table = lambda p: np.ctypeslib.as_array(p, shape=(m.num_lambda,))  # noqa: E731
    assert [table(m.sigma_ext)[idx], table(m.sigma_sca)[idx], table(m.asymmpar)[idx]] == list(gold["mix"][1:4])
    assert np.all(table(m.sigma_ext) == SIGMA_THOMSON) and np.all(table(m.sigma_sca) == SIGMA_THOMSON)
    assert np.all(table(m.sigma_abs) == 0.) and np.all(table(m.asymmpar) == 0.)
    assert sim.phase_functions[0] == PMC_PHASE_DIPOLE


def test_phase_functions_of_mixed_scenes():
    assert Simulation(ski("cfg2agnelec.ski")).setup().phase_functions == [PMC_PHASE_DIPOLE, PMC_PHASE_HG, PMC_PHASE_HG, PMC_PHASE_HG]
    assert Simulation(ski("cfg5elec.ski")).setup().phase_functions == [PMC_PHASE_HG, PMC_PHASE_DIPOLE, PMC_PHASE_HG, PMC_PHASE_HG]
    assert Simulation(ski("cfg2agn.ski")).setup().phase_functions == [PMC_PHASE_HG] * 4


def test_normalizations_give_the_same_medium(tmp_path):
    """the three normalizations of one electron box: the optical depth uses the Thomson cross section, the mass the electron mass"""
    text = open(ski("cfg1elec.ski")).read()
    pc = 3.08567758e16
    number = 1. / SIGMA_THOMSON * (2 * pc) ** 2     # optical depth 1 along 2 pc of a uniform box of (2 pc)^3: n = 1 / (sigma 2 pc)
    norm = re.search(r"<OpticalDepthMaterialNormalization[^>]*/>", text).group(0)
    dens = {}
    for tag, new in (("tau", norm), ("number", f'<NumberMaterialNormalization number="{number!r}"/>'),
                     ("mass", f'<MassMaterialNormalization mass="{number * 9.10938215e-31!r} kg"/>')):
        p = tmp_path / (tag + ".ski")
        p.write_text(text.replace(norm, new))
        sim = Simulation(str(p)).setup()
        h = scene_head(sim)
        dens[tag] = np.ctypeslib.as_array(h.medium.number_density, shape=(h.grid.num_cells,)).copy()
    assert np.allclose(dens["number"], dens["tau"], rtol=1e-14) and np.allclose(dens["mass"], dens["tau"], rtol=1e-14)
    assert np.allclose(dens["tau"], 1. / (SIGMA_THOMSON * 2 * pc), rtol=1e-12)


ELECTRON_MIX = 'includePolarization="false" includeThermalDispersion="false"'


@pytest.mark.parametrize("scene,old,new,message", [
    ("cfg1elec.ski", 'includePolarization="false"', 'includePolarization="true"', "ElectronMix with includePolarization"),
    ("cfg5elec.ski", 'includeThermalDispersion="false"', 'includeThermalDispersion="true"', "ElectronMix with includeThermalDispersion"),
    ("cfg1elec.ski", 'wavelengths="0.55 micron"', 'wavelengths="0.005 micron"', "ElectronMix with a source or instrument wavelength below"),
    ("cfg5elec.ski", 'minWavelength="0.1 micron" maxWavelength="10 micron" numWavelengths="20"',
     'minWavelength="0.005 micron" maxWavelength="10 micron" numWavelengths="20"', "ElectronMix with a source or instrument wavelength below"),
    ("cfg4small.ski", re.compile(r"<materialMix.*?</materialMix>"), f'<materialMix type="MaterialMix"><ElectronMix {ELECTRON_MIX}/></materialMix>',
     "ElectronMix in a ParticleMedium"),
])
def test_refused_electron_variants(tmp_path, scene, old, new, message):
    import os
    import shutil
    text = open(ski(scene)).read()
    changed = old.sub(new, text, count=1) if hasattr(old, "sub") else text.replace(old, new, 1)
    assert changed != text
    for f in os.listdir(os.path.dirname(ski(scene))):
        if f.endswith(".txt"):
            shutil.copy(ski(f), tmp_path)
    p = tmp_path / "refused.ski"
    p.write_text(changed)
    with pytest.raises(RuntimeError) as err:
        Simulation(str(p)).setup()
    assert "not supported" in str(err.value) and message in str(err.value)


def test_thermal_dispersion_is_ignored_in_an_oligochromatic_simulation(tmp_path):
    """ElectronMix.cpp:29: the reference switches dispersion off there, so the scene is that of cfg1elec"""
    text = open(ski("cfg1elec.ski")).read()
    p = tmp_path / "dispersion.ski"
    p.write_text(text.replace('includeThermalDispersion="false"', 'includeThermalDispersion="true"'))
    a, b = Simulation(str(p), num_packets=200).setup(), Simulation(ski("cfg1elec.ski"), num_packets=200).setup()
    assert a.phase_functions == b.phase_functions
    x, _ = O.run_primary(a, 0, 200, O.RNG_PHILOX, seed=3)
    y, _ = O.run_primary(b, 0, 200, O.RNG_PHILOX, seed=3)
    assert x.sum() > 0 and np.array_equal(x, y)


def test_scene_file_keeps_the_extension(tmp_path):
    n = 300
    sim = Simulation(ski("cfg2agnelec.ski"), num_packets=n).setup()
    path = str(tmp_path / "scene.bin")
    sim.save_scene(path)
    loaded = SceneFile(path)
    assert loaded.phase_functions == sim.phase_functions == [PMC_PHASE_DIPOLE, PMC_PHASE_HG, PMC_PHASE_HG, PMC_PHASE_HG]
    assert loaded.scene.ext and sim.scene.ext
    x, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=7)
    y, _ = O.run_primary(loaded, 0, n, O.RNG_PHILOX, seed=7)
    assert x.sum() > 0 and np.array_equal(x, y)
    # cfg5elec: the dipole in the second place
    other = Simulation(ski("cfg5elec.ski"), num_packets=n).setup()
    other.save_scene(path)
    assert SceneFile(path).phase_functions == [PMC_PHASE_HG, PMC_PHASE_DIPOLE, PMC_PHASE_HG, PMC_PHASE_HG]


def test_scene_file_without_extension_loads_as_henyey_greenstein(tmp_path):
    """a file written before scenes had an extension (tests/golden/cfg1nomed_scene_abi9_no_extension.bin, saved by the commit before this
    one) loads, every component Henyey-Greenstein; so does a file of today whose extension word is what it was then -- padding, zero"""
    old = SceneFile(golden("cfg1nomed_scene_abi9_no_extension.bin"))
    assert old.phase_functions == [PMC_PHASE_HG] * 4 and old.num_packets == 100
    assert scene_head(old).grid.num_cells == 1
    sim = Simulation(ski("cfg2agnelec.ski"), num_packets=100).setup()
    path = tmp_path / "scene.bin"
    sim.save_scene(str(path))
    data = bytearray(path.read_bytes())
    header = struct.Struct("<QiiQQqqiIQQQIIIIQ")
    fields = list(header.unpack_from(data))
    assert fields[8] == PMC_PHASE_DIPOLE      # (one byte per component, component 0 lowest)
    fields[8] = 0
    header.pack_into(data, 0, *fields)
    path.write_bytes(bytes(data))
    assert SceneFile(str(path)).phase_functions == [PMC_PHASE_HG] * 4


def test_unknown_phase_function_is_refused():
    """pmc_create_ext looks at the extension before it looks for a device: an unknown kind is PMC_ERR_UNSUPPORTED anywhere"""
    import ctypes as C
    from skirt9_amd import engine
    from skirt9_amd.host import SceneExt
    sim = Simulation(ski("cfg1elec.ski"), num_packets=10).setup()
    ext = SceneExt(C.sizeof(SceneExt), (C.c_int32 * 4)(7, 0, 0, 0))
    handle = C.c_void_p()
    rc = engine.lib().pmc_create_ext(int(sim.scene), C.addressof(ext), 0, C.byref(handle))
    assert rc == -2 and not handle.value
    assert "unknown phase function kind 7" in engine.lib().pmc_last_error().decode()
