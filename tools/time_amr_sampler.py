#!/usr/bin/env python3
"""Times the density sampler of an adaptive mesh medium (profiles/sweeps/amr_sampler.md): a mesh of --leaves cells from tools/make_amr.py
under the scene tests/ski/cfg6amr.ski,

  setup     Simulation.setup() with the densities on the host cores, and again with the device sampler (wall clock, the reading of the
            file included in both);
  sampler   MeshSampler.density on --positions random positions of the domain, --repeats times: wall clock per call, positions and
            results crossing PCIe included, scaled to 10^8 positions.

  python tools/time_amr_sampler.py --leaves 1000000 --depth 12 [--host-only]

Prints one line per figure.  The cell densities of both setups are compared bit for bit."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from skirt9_amd.host import Simulation, scene_head  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=1000000)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--positions", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-only", action="store_true", help="no device: the host setup alone")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        mesh_path = os.path.join(tmp, "mesh.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_amr.py"), "--preset", "disk", "--leaves", str(args.leaves),
                               "--depth", str(args.depth), mesh_path])
        text = open(os.path.join(ROOT, "tests", "ski", "cfg6amr.ski")).read().replace('filename="cfg6amr_mesh.txt"', 'filename="%s"' % mesh_path)
        ski = os.path.join(tmp, "timing.ski")
        open(ski, "w").write(text)

        def setup(device):
            sim = Simulation(ski)
            if device:
                sim.use_device_sampler(0)
            start = time.perf_counter()
            sim.setup()
            return sim, time.perf_counter() - start

        def densities(sim):
            head = scene_head(sim)
            return np.ctypeslib.as_array(head.medium.number_density, shape=(head.grid.num_cells,)).copy()

        host, seconds = setup(False)
        mesh = host.adaptive_mesh(0)
        print("mesh: %d nodes, %d leaves; spatial grid: %d cells" % (len(mesh["node_link"]), len(mesh["cell_density"]), len(densities(host))))
        print("setup, densities on the host cores (%d threads): %.2f s" % (os.cpu_count(), seconds))
        if args.host_only:
            return
        device, seconds = setup(True)
        print("setup, densities on the device: %.2f s" % seconds)
        print("cell densities equal bit for bit:", np.array_equal(densities(host).view(np.uint64), densities(device).view(np.uint64)))
        from skirt9_amd.engine import MeshSampler
        lo, hi = mesh["node_box"][0, :3], mesh["node_box"][0, 3:]
        points = lo + (hi - lo) * np.random.default_rng(1).random((args.positions, 3))
        sampler = MeshSampler(mesh, 0)
        sampler.density(points[:1024])
        for _ in range(args.repeats):
            start = time.perf_counter()
            sampler.density(points)
            seconds = time.perf_counter() - start
            print("sampler: %d positions in %.1f ms wall clock with transfers = %.0f ms per 1e8 positions" % (args.positions, 1e3 * seconds, 1e11 * seconds / args.positions))
        sampler.close()


if __name__ == "__main__":
    main()
