#!/usr/bin/env python3
"""Synthetic adaptive-mesh (AMR) dust disk for AdaptiveMeshMedium: a tree of nodes over a box domain, refined where the mass of a
double-exponential disk is, written as the SKIRT column text file that AdaptiveMeshSnapshot reads -- a line "! nx ny nz" for a node
that is subdivided, followed by its children (k outermost, i fastest), and a data row for a leaf.

  tools/make_amr.py --preset disk tests/ski/cfg6amr_mesh.txt       (the committed fixture: about 2500 leaves)
  tools/make_amr.py --preset sym  tests/ski/cfg6amrsym_mesh.txt    (the committed fixture: about 1500 leaves)
  tools/make_amr.py --preset disk --leaves 1000000 --depth 12 out.txt   (the timing mesh of profiles/sweeps/amr_sampler.md; not committed)

disk: a domain that is NOT symmetric about the origin and not dyadic, root 3 x 4 x 2, refinements drawn from 2x2x2, 3x2x1 and 1x1x2.
sym:  a domain symmetric about the origin, root 4 x 4 x 4, 2x2x2 refinements only: the coordinate planes are cell walls at every level.

The leaf with the largest mass is refined next until the number of leaves is reached, down to --depth levels below the root.  Rows hold
three columns WITHOUT a unit header, so that the same file serves every massType with the default unit of its first column: the density
(Msun/pc3 as a mass density, 1/cm3 as a number density; a bare number as a Number), the metallicity, the temperature (K).  A few leaves
carry density 0 and a few are hot (10^6 K: above any dust temperature cutoff).  Deterministic for a given (preset, leaves, depth, seed,
numpy version)."""
import argparse
import heapq

import numpy as np

PRESETS = {
    # extent (pc): xmin, ymin, zmin, xmax, ymax, zmax; root subdivision; refinement kinds
    "disk": ((-19000., -16500., -3700., 17000., 18300., 3100.), (3, 4, 2), ((2, 2, 2), (3, 2, 1), (1, 1, 2)), 2500, 5),
    "sym": ((-16000., -16000., -4000., 16000., 16000., 4000.), (4, 4, 4), ((2, 2, 2),), 1500, 4),
}


def disk_density(x, y, z, hr, hz, rho0):
    return rho0 * np.exp(-np.hypot(x, y) / hr - abs(z) / hz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--preset", choices=sorted(PRESETS), default="disk")
    ap.add_argument("--leaves", type=int, default=0, help="leaves to reach (default: the preset's)")
    ap.add_argument("--depth", type=int, default=0, help="deepest level below the root (default: the preset's)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--hr", type=float, default=4000.0, help="scale length (pc)")
    ap.add_argument("--hz", type=float, default=250.0, help="scale height (pc)")
    ap.add_argument("--rho0", type=float, default=3.2e-4, help="central density (Msun/pc3): tau_z(0.55 micron) ~ 1 at kappa 3000 m2/kg")
    args = ap.parse_args()
    extent, root, kinds, leaves, depth = PRESETS[args.preset]
    leaves = args.leaves or leaves
    depth = args.depth or depth
    rng = np.random.default_rng(args.seed)

    # nodes as lists: box, level, children (None: leaf)
    box, level, children = [extent], [0], [None]

    def mass(n):
        b = box[n]
        c = [0.5 * (b[a] + b[a + 3]) for a in range(3)]
        return disk_density(c[0], c[1], c[2], args.hr, args.hz, args.rho0) * (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])

    def refine(n, dims):
        b = box[n]
        nx, ny, nz = dims
        first = len(box)
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    box.append((b[0] + i * (b[3] - b[0]) / nx, b[1] + j * (b[4] - b[1]) / ny, b[2] + k * (b[5] - b[2]) / nz,
                                b[0] + (i + 1) * (b[3] - b[0]) / nx, b[1] + (j + 1) * (b[4] - b[1]) / ny, b[2] + (k + 1) * (b[5] - b[2]) / nz))
                    level.append(level[n] + 1)
                    children.append(None)
        children[n] = (dims, first)
        return range(first, first + nx * ny * nz)

    heap = []
    count = 1
    for c in refine(0, root):
        heapq.heappush(heap, (-mass(c), c))
    count += len(box) - 2
    while heap and count < leaves:
        _, n = heapq.heappop(heap)
        dims = kinds[int(rng.integers(len(kinds)))]
        for c in refine(n, dims):
            if level[c] < depth:
                heapq.heappush(heap, (-mass(c), c))
        count += dims[0] * dims[1] * dims[2] - 1

    lines = []
    num_leaves = 0
    stack = [0]
    while stack:  # depth first, children in order
        n = stack.pop()
        if children[n] is None:
            b = box[n]
            c = [0.5 * (b[a] + b[a + 3]) for a in range(3)]
            rho = disk_density(c[0], c[1], c[2], args.hr, args.hz, args.rho0)
            u = rng.random(3)
            if u[0] < 0.01:
                rho = 0.
            temperature = 1e6 if u[1] < 0.01 else 10. ** (2. + 2. * u[2])
            metallicity = 0.01 + 0.02 * rng.random()
            lines.append("%.9g %.6g %.6g" % (rho, metallicity, temperature))
            num_leaves += 1
        else:
            (nx, ny, nz), first = children[n]
            lines.append("! %d %d %d" % (nx, ny, nz))
            stack.extend(range(first + nx * ny * nz - 1, first - 1, -1))
    with open(args.out, "w") as fh:
        fh.write("# synthetic adaptive mesh dust disk (tools/make_amr.py --preset %s --leaves %d --depth %d --seed %d): %d leaves\n"
                 % (args.preset, leaves, depth, args.seed, num_leaves))
        fh.write("# domain (pc): %s\n" % " ".join("%g" % v for v in extent))
        fh.write("# per leaf: density (Msun/pc3 | 1/cm3 | number), metallicity, temperature (K); no unit header: default units\n")
        fh.write("\n".join(lines) + "\n")
    print(args.out, num_leaves, "leaves,", len(box), "nodes, deepest level", max(level))


if __name__ == "__main__":
    main()
