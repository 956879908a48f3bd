"""What tests/test_host_temperature.py, tests/test_gpu_temperature.py and tests/golden/make_golden_temperature.py share: the golden scenes of
the dust temperature probes and what their fixtures must show, the numpy restatement of the energy balance per cell, the weighted path sum
that defines an average along a ray, and random tables and special rows for the kernel."""
import functools
import gzip

import numpy as np

import probe_checks as P

GOLDEN_SCENES = ["cfg1temp", "cfg3temp", "cfg3mmtemp", "cfg2bintemp"]  # Cartesian, octree, octree with three components, binary tree

golden_files = P.golden_files


def per_cell_values(path):
    """the value columns of a per-cell text file (gzipped or not): [num_cells][columns]"""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        rows = [line.split() for line in f if not line.startswith("#")]
    table = np.array(rows, dtype=np.float64)
    assert np.array_equal(table[:, 0], np.arange(len(table)))
    return table[:, 1:]


def fits_image(path):
    """the pixels of a plain FITS image written by the reference (BITPIX -32, NAXIS 2): [ny][nx]"""
    data = open(path, "rb").read()
    cards = {}
    at = 0
    while True:
        card = data[at:at + 80].decode()
        at += 80
        if card.startswith("END"):
            break
        if "=" in card[:10]:
            cards[card[:8].strip()] = card[10:].split("/")[0].strip()
    assert int(cards["BITPIX"]) == -32 and int(cards["NAXIS"]) == 2
    nx, ny = int(cards["NAXIS1"]), int(cards["NAXIS2"])
    start = (at + 2879) // 2880 * 2880
    return np.frombuffer(data[start:start + 4 * nx * ny], dtype=">f4").reshape(ny, nx).astype(np.float64)


def assert_golden_is_meaningful(name):
    """every per-cell temperature file has T > 0 in at least 95 % of its cells, every map is nonzero in at least half of its pixels, the
    file of cfg3mmtemp's second dust component has cells with and without a temperature, and the field and the absorbed luminosity are not
    empty; returns what was found per file"""
    files = golden_files(name)
    facts = {}
    kinds = set()
    for f, path in files.items():
        if f.endswith("_T.dat"):
            T = per_cell_values(path)[:, 0]
            share = (T > 0).mean()
            facts[f] = f"{len(T)} cells, T > 0 in {100 * share:.2f} %, max {T.max():.3f} K"
            if name == "cfg3mmtemp" and f.endswith("_1_T.dat"):
                assert (T == 0).any() and (T > 0).any(), f
                kinds.add("partial")
            else:
                assert share >= 0.95, (f, share)
            kinds.add("cells")
        elif f.endswith("_T.fits"):
            image = fits_image(path)
            share = (image != 0).mean()
            facts[f] = f"{image.shape[1]} x {image.shape[0]} pixels, {100 * share:.1f} % nonzero, max {image.max():.3f} K"
            assert share >= 0.5, (f, share)
            kinds.add("map")
        elif f.endswith("_Labs.dat") or f.endswith("_J.dat"):
            values = per_cell_values(path)
            facts[f] = f"{values.shape[0]} cells x {values.shape[1]} bins, {100 * (values > 0).mean():.1f} % nonzero"
            assert (values > 0).mean() > 0.5, f
            kinds.add(f[-8:])
        else:
            raise AssertionError(f"unexpected fixture {f}")
    assert {"cells", "map", "Labs.dat", "rf_J.dat"} <= kinds, (name, kinds)
    if name == "cfg3mmtemp":
        assert "partial" in kinds
    return facts


# ---- the energy balance restated with numpy

def numpy_temperatures(tables, rf):
    """[H + 1][num_cells] as skh_dust_temperatures / pmc_dust_temperatures define it (include/pmc.h): element-wise IEEE operations (numpy does
    not contract), the sum over the bins from the last one down to the first, the table lookup of NR::clampedValue<interpolateLinLin>"""
    width, sigma, planck, Tv = tables["width"], tables["sigma"], tables["planckabs"], tables["temperature"]
    factor, rho = tables["cell_factor"], tables["mass_density"]
    H, L = sigma.shape
    cells = factor.size
    rf = np.asarray(rf, dtype=np.float64).reshape(cells, L)
    J = rf * factor[:, None] / width[None, :]
    out = np.zeros((H + 1, cells))
    sum_rho_t, sum_rho = np.zeros(cells), np.zeros(cells)
    n = Tv.size
    for h in range(H):
        total = sigma[h, L - 1] * J[:, L - 1] * width[L - 1]
        for ell in range(L - 2, -1, -1):
            total = total + sigma[h, ell] * J[:, ell] * width[ell]
        xv = planck[h]
        # NR::locate: n - 2 at the last node, else the last index whose node is not above x (n - 1 beyond the table)
        i = np.searchsorted(xv, total, side="right") - 1
        i = np.where(total == xv[n - 1], n - 2, i)
        inside = np.clip(i, 0, n - 2)
        x1, x2, f1, f2 = xv[inside], xv[inside + 1], Tv[inside], Tv[inside + 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            value = f1 + ((total - x1) / (x2 - x1)) * (f2 - f1)
        value = np.where(i < 0, Tv[0], np.where(i >= n - 1, Tv[n - 1], value))
        T = np.where((rho[h] > 0) & (total > 0), value, 0.)
        out[h] = T
        has = rho[h] > 0
        sum_rho_t = np.where(has, sum_rho_t + rho[h] * T, sum_rho_t)
        sum_rho = np.where(has, sum_rho + rho[h], sum_rho)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[H] = np.where(sum_rho > 0, sum_rho_t / sum_rho, 0.)
    return out


def inputs(tables, rf):
    """the left-hand side of the energy balance, [H][num_cells], summed as numpy_temperatures sums it"""
    width, sigma, factor = tables["width"], tables["sigma"], tables["cell_factor"]
    H, L = sigma.shape
    rf = np.asarray(rf, dtype=np.float64).reshape(factor.size, L)
    J = rf * factor[:, None] / width[None, :]
    result = []
    for h in range(H):
        total = sigma[h, L - 1] * J[:, L - 1] * width[L - 1]
        for ell in range(L - 2, -1, -1):
            total = total + sigma[h, ell] * J[:, ell] * width[ell]
        result.append(total)
    return np.array(result)


def random_tables(num_cells, num_lambda, H, seed, num_temperatures=1001):
    """tables of the shape and magnitude of a simulation's, from a seeded generator: H dust components, every third cell of the components
    behind the first without mass"""
    rng = np.random.default_rng(seed)
    Tv = np.concatenate([[0.], np.sort(rng.random(num_temperatures - 1)) * 4999. + 1e-3])
    Tv[-1] = 5000.
    planck = np.zeros((H, num_temperatures))
    for h in range(H):
        planck[h, 1:] = np.cumsum(rng.random(num_temperatures - 1) + 0.01) * 1e-27
    rho = rng.random((H, num_cells)) * 1e-22
    for h in range(1, H):
        rho[h, h::3] = 0.
    return {"width": rng.random(num_lambda) * 1e-6 + 1e-8, "sigma": rng.random((H, num_lambda)) * 1e-24 + 1e-27, "planckabs": planck,
            "temperature": Tv, "cell_factor": 1. / (4. * np.pi * (rng.random(num_cells) * 1e54 + 1e50)), "mass_density": rho}


def special_rows(tables, rf, seed):
    """rf with special rows placed in cell 0, in the last cell and at indices that are no multiple of 64 (which kinds get the two end cells
    turns with the seed; every kind has a cell off the multiples of 64): all zero (T = 0); an
    input above the last node of every component's table (exactly the last temperature); an input between 0 and the first node above it; an
    input that EQUALS a node of component 0's table exactly (a one-hot row; the node of the caller's table is MOVED onto the row's input, by a
    rounding error).  Returns (rf, {kind: cells}); what each kind yields is asserted by the caller on the restatement"""
    rf = np.array(rf, dtype=np.float64).reshape(tables["cell_factor"].size, -1)
    cells, L = rf.shape
    rng = np.random.default_rng(seed)
    width, sigma, planck, factor = tables["width"], tables["sigma"], tables["planckabs"], tables["cell_factor"]
    # every kind has a cell whose index is no multiple of 64 (65, 129, 67, 131); cell 0 and the last cell go to two of the kinds, which two
    # turns with the seed: over four consecutive seeds every kind has been in both
    spots = {"zero": [5, 65], "hot": [6, 129], "faint": [1, cells - 2, 67], "node": [2, cells - 3, 131]}
    kinds = list(spots)
    spots[kinds[seed % 4]][0] = 0
    last = kinds[(seed + 1) % 4]
    spots[last][1 if len(spots[last]) == 3 else 0] = cells - 1
    assert cells > 140
    for m in spots["zero"]:
        rf[m] = 0.
    for m in spots["hot"]:
        rf[m] = rng.random(L) + 0.5
        rf[m] *= 4. * planck[:, -1].max() / inputs(tables, rf)[:, m].min()
    for m in spots["faint"]:
        rf[m] = rng.random(L) + 0.5
        rf[m] *= 0.25 * planck[:, 1].min() / inputs(tables, rf)[:, m].max()
    for j, m in enumerate(spots["node"]):
        # a one-hot row whose input lies within rounding of a node; the node then takes the row's input, to the bit (the table stays ascending:
        # its nodes are 1e-29 apart at the least, the move is one of 1e-16 of the node)
        node = 100 + 37 * j
        ell = (L - 1) if j % 2 else 0
        rf[m] = 0.
        rf[m, ell] = planck[0, node] / (sigma[0, ell] * factor[m])
        exact = inputs(tables, rf)[0, m]
        assert planck[0, node - 1] < exact < planck[0, node + 1] and abs(exact / planck[0, node] - 1.) < 1e-14
        planck[0, node] = exact
    return rf.reshape(-1), spots


# ---- averages along rays

def weighted_path_sum(m, ds, w, q):
    """[1 + V]: per segment with m >= 0, in path order, weight = ds * w[m]; sum[0] += weight; sum[1 + v] += weight * q[v][m] -- one IEEE
    product, one sum, one product and one sum (numpy's element-wise operations do not contract)"""
    total = np.zeros(1 + q.shape[0])
    for cell, length in zip(m.tolist(), ds.tolist()):
        if cell >= 0:
            weight = length * w[cell]
            total[0] = total[0] + weight
            total[1:] = total[1:] + weight * q[:, cell]
    return total


def oracle_weighted_integrator(sim, cap=65536):
    """the `weighted` callable of Simulation.write_probes over the test oracle's ray segments"""
    import oracle_lib as O

    def weighted(origins, directions, w, q):
        sums = np.zeros((len(origins), 1 + q.shape[0]))
        for i in range(len(origins)):
            m, ds = O.trace_ray(sim, origins[i], directions[i], cap=cap)
            assert len(m) < cap
            sums[i] = weighted_path_sum(m, ds, w, q)
        return sums

    return weighted


@functools.lru_cache(maxsize=None)
def oracle_field(name):
    """(sim, rf): the scene set up and the radiation field of the test oracle with the reference's random stream, computed once per scene"""
    import oracle_lib as O
    from conftest import ski
    from skirt9_amd.host import Simulation
    sim = Simulation(ski(name + ".ski")).setup()
    _, rf, counters = O.run_primary_rf(sim, 0, sim.num_packets, O.RNG_MT19937, ext=True)
    assert counters.histories == sim.num_packets
    rf.setflags(write=False)
    return sim, rf
