"""The borders of the sweep over slot runs that the transition and launch kernels share (run on the MI355X box with `pytest -m gpu`).

Both kernels serve the slots of a group in runs of 256 per wave, 1024 per workgroup and tile of the grid (transitionBody in
pmc_transition.inc, launchBody in pmc_launch.inc).  The slot counts below are the smallest that meet every border of that sweep: a partial wave tile (1, 63,
65), a full and a partial run of 256 (255, 256, 257), a full and a partial workgroup span (1023, 1024, 1025), a second tile (2049).  With
4000 histories a slot is refilled between twice and 4000 times, so the compaction of the ended slots, the scan of their counts and the
assignment of the history indices all run across those borders, and the end of every segment runs over the list of live slots.  Scenes: one
per flavour of the transition kernel (plain, dipole, moving source) and a Voronoi grid.

Every run is compared with the oracle's frames of the same 4000 histories (computed once per scene), with the tolerances of
test_gpu_slot_reuse.  And the runs of a scene are compared with each other where the result is exact on integers and does not depend on
the order of the atomic additions (as test_sparse_generations_equal_the_slot_order_generations does): the counted histories, paths,
scatterings and detector updates, and the number of contributing histories per bin (the k = 0 statistics array) are equal for every slot
count -- each run is held against the scene's run in 1025 slots.
"""
import numpy as np
import pytest

from conftest import ski
from test_gpu_parity import _pixel_shapes
from test_gpu_slot_reuse import _run_and_compare, _sim

pytestmark = pytest.mark.gpu

N = 4000
SLOTS = (1, 63, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
BASE = 1025
# scene: (the oracle follows the scene's extension -- dipole phase function, moving source --, two wavelength bins per history --
# a moving source: _compare_frames --, slot counts)
SCENES = {"cfg2small.ski": (False, False, SLOTS), "cfg1elec.ski": (True, False, SLOTS), "cfg1kin.ski": (True, True, SLOTS),
          "cfg5small.ski": (False, False, (63, 257, 1025))}
EXACT = ("histories", "paths", "scatterings", "detector_updates")

_runs = {}


def _run(name, slots):
    """counters and per-bin numbers of contributing histories of the scene in `slots` slots, after the comparison with the oracle: once per module"""
    key = (name, slots)
    if key not in _runs:
        gpu, c = _run_and_compare(ski(name), name, N, slots, ext=SCENES[name][0], two_bins_per_history=SCENES[name][1])
        sim = _sim(ski(name), N)
        counts = []
        for inst in range(len(_pixel_shapes(sim))):
            lay = sim.layout(inst)
            if lay.wifu_offset >= 0:
                counts.append(gpu[lay.wifu_offset:lay.wifu_offset + lay.npix * lay.num_lambda].copy())
        assert counts and sum(a.sum() for a in counts) > 0
        _runs[key] = ({k: c[k] for k in EXACT}, counts)
    return _runs[key]


@pytest.mark.parametrize("name,slots", [(name, s) for name, (_, _, counts) in SCENES.items() for s in counts])
def test_scene_at_the_borders_of_the_slot_runs(name, slots):
    counters, counts = _run(name, slots)
    base_counters, base_counts = _run(name, BASE)
    print(name, slots, counters)
    assert counters == base_counters
    for a, b in zip(counts, base_counts):
        assert np.array_equal(a, b)
