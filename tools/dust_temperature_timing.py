#!/usr/bin/env python3
"""Kernel time of pmc_dust_temperatures on the headline octree (tests/ski/cfg3.ski: the 953 688-cell octree, panchromatic) with the field stored
on 6 and on 50 bins, next to skh_dust_temperatures on the same table on one host thread: what profiles/sweeps/dust_temperature.md records.

  python tools/dust_temperature_timing.py [result.json]

Needs an MI355X.  One JSON line per field grid on standard output."""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
os.environ["SKH_THREADS"] = "16"
from skirt9_amd.engine import Engine
from skirt9_amd.host import Simulation, scene_head

GRID = ('<RadiationFieldOptions storeRadiationField="true"><radiationFieldWLG type="DisjointWavelengthGrid"><LogWavelengthGrid '
        'minWavelength="0.15 micron" maxWavelength="8 micron" numWavelengths="%d"/></radiationFieldWLG></RadiationFieldOptions>')
out = []
for bins in (6, 50):
    text = open(os.path.join(ROOT, "tests", "ski", "cfg3.ski")).read()
    a, b = text.index("<RadiationFieldOptions"), text.index("</radiationFieldOptions>")
    path = os.path.join(tempfile.mkdtemp(), f"cfg3rf{bins}.ski")
    open(path, "w").write(text[:a] + GRID % bins + text[b:])
    t0 = time.time()
    sim = Simulation(path, num_packets=200000).setup()
    t1 = time.time()
    tables = sim.temperature_tables()
    t2 = time.time()
    eng = Engine(sim.scene, 0)
    eng.run_primary(0, 200000, 1)
    rf = eng.download_radiation_field()
    ms, wall = [], []
    for _ in range(5):
        t = time.time()
        gpu = eng.dust_temperatures(tables)
        wall.append(time.time() - t)
        ms.append(eng.last_temperature_ms())
    os.environ["SKH_THREADS"] = "1"  # (one host thread)
    t = time.time()
    cpu = sim.dust_temperatures(rf)
    t_one = time.time() - t
    same = bool(np.array_equal(gpu.view(np.uint64), cpu.view(np.uint64)))
    row = {"bins": bins, "cells": int(scene_head(sim).grid.num_cells), "setup_s": round(t1 - t0, 2), "tables_s": round(t2 - t1, 3),
           "kernel_ms": [round(x, 4) for x in ms], "call_wall_ms": [round(1e3 * x, 2) for x in wall], "host_one_thread_s": round(t_one, 3),
           "bit_identical": same, "cells_with_T": float((gpu[-1] > 0).mean()), "T_max": float(gpu[-1].max())}
    print(json.dumps(row), flush=True)
    out.append(row)
    eng.close()
    os.environ["SKH_THREADS"] = "16"
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
