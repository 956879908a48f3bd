#!/usr/bin/env python3
"""Octree against binary tree on the full-size scene of tests/ski/cfg2.ski (profiles/sweeps/bintree_vs_octree.txt).

  python tools/bintree_vs_octree.py [--packets 1e8] [--steps 3] [--parent-library PATH]

Three forms of the scene, each in a process of its own (the engine library is loaded once per process):
  octree       tests/ski/cfg2.ski as it is: the octree kernels
  as-bintree   the same octree scene with the switch PMC_TREE_AS_BINTREE: the binary tree's tables and kernels on the octree's cells --
               the cost of the new step without the change of the grid
  bintree      a copy of the ski file with treeType="BinTree" and the two levels of the policy times three
and, with --parent-library, `octree` once more on an engine library built from the parent commit (measured in the same session).
Per form: the cell count, counted cell visits per history, and packets/s from pmc_last_timing (HIP events around the segment) over
`--packets` histories per step: one warm-up step, then `--steps` timed ones (median and spread).  Prints one JSON line per form.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SKI = os.path.join(ROOT, "tests", "ski", "cfg2.ski")


def bintree_ski(tmp):
    text = open(SKI).read()
    policy = re.search(r'minLevel="(\d+)" maxLevel="(\d+)"', text)
    assert 'treeType="OctTree"' in text and policy
    text = text.replace('treeType="OctTree"', 'treeType="BinTree"')
    text = text.replace(policy.group(0), f'minLevel="{3 * int(policy.group(1))}" maxLevel="{3 * int(policy.group(2))}"')
    path = os.path.join(tmp, "cfg2bintree.ski")
    open(path, "w").write(text)
    return path


def measure(form, ski, packets, steps):
    import time
    import numpy as np
    from skirt9_amd.engine import Engine, clear_tuning, set_tuning
    from skirt9_amd.host import Simulation, scene_head
    t0 = time.time()
    sim = Simulation(ski, num_packets=packets).setup()
    setup_s = time.time() - t0
    if form == "as-bintree":
        set_tuning("PMC_TREE_AS_BINTREE")
    eng = Engine(sim.scene, 0)
    clear_tuning()
    eng.run_primary(0, packets, 1)  # warm-up
    eng.sync()
    eng.clear()
    eng.reset_counters()
    ms = []
    for step in range(steps):
        eng.run_primary(step * packets, packets, 1)
        eng.sync()
        ms.append(eng.last_timing()["total_ms"])
    c = eng.counters()
    frames = eng.download()
    ms.sort()
    median = ms[len(ms) // 2]
    grid = scene_head(sim).grid
    return {"form": form, "cells": int(grid.num_cells), "nodes": int(grid.num_nodes), "max_level": int(np.ctypeslib.as_array(grid.node_level, shape=(grid.num_nodes,)).max()),
            "packets_per_step": packets, "steps": steps, "segment_ms": ms, "packets_per_s": packets / (median * 1e-3),
            "cell_visits_per_history": c["cell_visits"] / c["histories"], "rewalk_visits_per_history": c["rewalk_visits"] / c["histories"],
            "paths_per_history": c["paths"] / c["histories"], "scatterings_per_history": c["scatterings"] / c["histories"],
            "frames_sum": float(frames.sum()), "host_setup_s": round(setup_s, 1), "library": os.environ.get("PMC_LIBRARY", "this tree")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=float, default=1e8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="libpmc.so built from the parent commit: the octree form is measured on it as well")
    ap.add_argument("--form", default=None, help="(internal) measure this form in this process")
    ap.add_argument("--ski", default=SKI)
    args = ap.parse_args()
    packets = int(args.packets)
    if args.form:
        print(json.dumps(measure(args.form, args.ski, packets, args.steps)), flush=True)
        return
    with tempfile.TemporaryDirectory() as tmp:
        runs = [("octree", SKI, None), ("as-bintree", SKI, None), ("bintree", bintree_ski(tmp), None)]
        if args.parent_library:
            runs.insert(1, ("octree", SKI, args.parent_library))
        for form, ski, library in runs:
            env = dict(os.environ)
            if library:
                env["PMC_LIBRARY"] = os.path.abspath(library)
            # (a fresh process per form; a failed one ends the series: nothing more is started on the device)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--form", form, "--ski", ski, "--packets", str(packets), "--steps", str(args.steps)],
                           env=env, check=True, timeout=900)


if __name__ == "__main__":
    main()
