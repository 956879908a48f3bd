"""Launch kernel flavours against the generic launch kernel (run on the MI355X box with `pytest -m gpu`).

The launch kernel is compiled once per launch flavour (skirt9_amd/csrc/pmc_device.h PMC_LAUNCH_*: what the scene's sources fix of
SourceSystem::launch -- oligochromatic or sampled wavelengths, the geometry set, isotropic emission or not, a moving source) and once in its
generic form, which asks the source for everything; the switch PMC_LAUNCH_GENERIC runs the generic form whatever the scene is.  A flavour only
leaves code out: it draws the same deviates in the same order, so every history must come out as the generic kernel launches it.  Here each
scene runs twice on one device, with the flavour it selects and with the generic kernel, in a pool far smaller than the number of histories
(every slot is refilled several times, through the persistent first fill and through the refills), and
  * every integer counter is EQUAL: histories, paths, cell visits, detector updates, scatterings;
  * the frames agree to the tolerances of test_gpu_parity (_compare_frames: totals 1e-9, elements 1e-6) -- the order in which the detector
    atomics arrive differs from run to run, so the sums are not bit-identical.
"""
import pytest

from conftest import ski
from skirt9_amd.engine import set_tuning
from skirt9_amd.host import Simulation
from test_gpu_parity import _compare_frames

pytestmark = pytest.mark.gpu

SEED = 314159
KIN, OLIGO, ISOTROPIC, GEOM_SHIFT = 1, 2, 4, 3   # pmc_device.h PMC_LAUNCH_*
SERSIC, POINT = 1, 2
COUNTERS = ("histories", "paths", "cell_visits", "detector_updates", "scatterings")

_sims = {}


def _sim(name, n):
    if (name, n) not in _sims:
        _sims[(name, n)] = Simulation(ski(name), num_packets=n).setup()
    return _sims[(name, n)]


def _run(sim, n, generic):
    """histories [0, n) of the scene; returns (frames, counters, flavour, generations)"""
    from skirt9_amd.engine import Engine
    set_tuning("PMC_LAUNCH_GENERIC", "1" if generic else None)
    eng = Engine(sim.scene, 0)
    flavour = eng.launch_flavour()
    eng.run_primary(0, n, SEED)
    frames = eng.download()
    c = eng.counters()
    generations = eng.last_timing()["generations"]
    eng.close()
    set_tuning("PMC_LAUNCH_GENERIC", None)
    return frames, c, flavour, generations


def _both(name, n, slots, groups, monkeypatch, kin=False):
    monkeypatch.setenv("PMC_NUM_SLOTS", str(slots))    # (read by pmc_create)
    monkeypatch.setenv("PMC_NUM_GROUPS", str(groups))
    sim = _sim(name, n)
    special, c1, flavour, generations = _run(sim, n, False)
    generic, c0, generic_flavour, _ = _run(sim, n, True)
    assert generic_flavour == (KIN if kin else 0)
    assert c0["histories"] == n and c0["stat_overflows"] == 0
    for key in COUNTERS:
        assert c1[key] == c0[key], (key, c1[key], c0[key])
    assert c1["stat_overflows"] == 0
    _compare_frames(sim, special, generic, n, two_bins_per_history=kin)
    return flavour, generations


# scene, (bits that must be set, bits that must be clear, geometry set); None: the generic kernel
SCENES = [("cfg2small.ski", (OLIGO | ISOTROPIC, KIN, SERSIC)),   # the headline flavour: oligochromatic, one Sersic source
          ("cfg1.ski", (OLIGO | ISOTROPIC, KIN, POINT)),         # a point source
          ("cfg3small.ski", (ISOTROPIC, OLIGO | KIN, SERSIC)),   # a sampled SED with a wavelength bias (black body: analytic specific luminosity)
          ("cfg3norm.ski", (ISOTROPIC, OLIGO | KIN, SERSIC)),    # a wavelength bias weighted by a tabulated SED
          ("cfg3multi.ski", None),                               # three sources of mixed kinds: no flavour covers them
          ("cfg1con.ski", (0, ISOTROPIC | KIN, POINT)),          # an anisotropic point source (emission into a double cone)
          ("cfg1laser.ski", (0, ISOTROPIC | KIN, POINT)),        # ... and a laser
          ("cfg1kin.ski", (KIN | ISOTROPIC, OLIGO, POINT))]      # a moving point source


@pytest.mark.parametrize("name,expect", SCENES)
def test_flavour_launches_the_histories_of_the_generic_kernel(name, expect, monkeypatch):
    """20 000 histories in 4096 slots (PMC_NUM_SLOTS; PMC_NUM_GROUPS = 3, of which a pool below 3 x 65536 slots makes one group): five
    generations' worth of refills at least"""
    n = 20000
    kin = "kin" in name
    flavour, generations = _both(name, n, 4096, 3, monkeypatch, kin=kin)
    assert generations >= n / 4096
    if expect is None:
        assert flavour == 0
    else:
        on, off, geometry = expect
        assert flavour & on == on and flavour & off == 0 and flavour >> GEOM_SHIFT == geometry, flavour
        assert flavour not in (0, KIN)


@pytest.mark.parametrize("name", ["cfg2small.ski", "cfg3small.ski"])
@pytest.mark.parametrize("n", [3000, 4096])
def test_first_fill_alone(name, n, monkeypatch):
    """fewer histories than the 4096 slots (the segment's pool is then as large as its histories; 3000 is no multiple of 64 or 256: the
    first fill ends in a partial wave tile of a partial run), and exactly as many histories as slots: the first fill launches all of them, and
    no slot is ever refilled"""
    _both(name, n, 4096, 3, monkeypatch)


def test_three_slot_groups(monkeypatch):
    """the headline flavour in three real slot groups (196 613 slots, just above the 3 x 65536 below which a pool is one group; the last
    group is smaller than the others and ends in a partial wave tile), each filled by its own persistent launch workgroups over one history
    cursor and refilled about twice"""
    n = 500000
    flavour, generations = _both("cfg2small.ski", n, 196613, 3, monkeypatch)
    assert flavour == OLIGO | ISOTROPIC | (SERSIC << GEOM_SHIFT)
    assert generations >= n / 196613
