"""AdaptiveMeshMedium on the host (skirt9_amd/host/adaptive_mesh.cpp): the snapshot's tables and densities against the pure-Python restatement
of tests/amr_checks.py bit for bit, the sampled cell densities, output files, convergence info and density cuts against what the UNMODIFIED
reference recorded (tests/golden/make_golden_amr.py), the mass types against hand-computed values, and the reader's and the file's errors by
their words.  No GPU."""
import hashlib
import os

import numpy as np
import pytest

import amr_checks as A
import convergence_checks as K
import oracle_lib as O
from conftest import golden, ski
from skirt9_amd.host import Simulation, scene_head
from test_host_convergence import _oracle_integrator, _python_sampler
from test_oracle_golden import _same_file

FIXTURES = {"cfg6amr": ("cfg6amr_mesh.txt", A.DISK_EXTENT_PC), "cfg6amrconv": ("cfg6amrsym_mesh.txt", A.SYM_EXTENT_PC)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_mesh(got, want):
    for key in ("node_dims", "node_link"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("node_box", "cell_density"):
        assert got[key].shape == want[key].shape and np.array_equal(_bits(got[key]), _bits(want[key])), key


def _assert_table_rules(mesh):
    """root = node 0, every parent before its children, the children of a node consecutive, every node but the root the child of one parent"""
    dims, link = mesh["node_dims"], mesh["node_link"]
    parents = np.zeros(len(link), dtype=np.int64)
    for n in range(len(link)):
        if dims[n, 0]:
            assert (dims[n] >= 1).all() and link[n] > n
            parents[link[n]:link[n] + int(np.prod(dims[n]))] += 1
        else:
            assert (dims[n] == 0).all()
    assert parents[0] == 0 and (parents[1:] == 1).all()
    leaves = link[dims[:, 0] == 0]
    assert sorted(leaves.tolist()) == list(range(len(mesh["cell_density"])))


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_tables_and_densities_equal_the_restatement(name):
    """the tree the host builds from the file is the restatement's, box for box; the density at every point of the point sets is the
    restatement's, and the restatement locates every one of them"""
    sim = Simulation(ski(name + ".ski")).setup()
    mesh = sim.adaptive_mesh(0)
    file_name, extent_pc = FIXTURES[name]
    builder, units = A.read_mesh_file(ski(file_name), [v * A.PC for v in extent_pc])
    assert units == []  # (no unit header: the default unit Msun/pc3)
    want = builder.tables([row[0] * (A.MSUN / A.PC ** 3) for row in builder.rows])
    _assert_same_mesh(mesh, want)
    _assert_table_rules(mesh)
    assert len(mesh["cell_density"]) == (2502 if name == "cfg6amr" else 1506)
    assert A.leaf_levels(mesh).max() == (5 if name == "cfg6amr" else 4)
    sets = A.point_sets(mesh, upper_walls=False)
    for what, points in sets.items():
        assert A.cannot_locate(mesh, points) == [], what
        got = sim.imported_densities(0, points)
        assert np.array_equal(_bits(got), _bits(A.Descent(mesh).densities(points))), what
    assert len(sets["walls"]) > 4000 and len(sets["near_walls"]) > 24000
    assert (sim.imported_densities(0, sets["outside"]) == 0).all() and (sim.imported_densities(0, sets["odd"]) == 0).all()
    assert (sim.imported_densities(0, sets["centres"]) == mesh["cell_density"]).all()


def _synthetic_simulation(tmp_path, kind):
    mesh = A.SYNTHETIC[kind]()
    path = str(tmp_path / (kind + "_mesh.txt"))
    A.write_mesh_file(mesh, path)
    extent = mesh["node_box"][0].tolist()
    sim = Simulation(A.mesh_ski(tmp_path, kind, path, extent)).setup()
    builder, units = A.read_mesh_file(path, extent)
    assert units == ["kg/m3"]
    return sim, builder.tables([row[0] for row in builder.rows])


@pytest.mark.parametrize("kind", list(A.SYNTHETIC))
def test_synthetic_meshes_equal_the_restatement(kind, tmp_path):
    """a single leaf, 2x2x2, a chain refined 30 levels into one corner, a 3x2x1 nest: written as files with a unit header, read by the host,
    and sampled at the point sets -- on the dyadic meshes with the points ON the outer upper walls of the domain, which belong to it"""
    sim, want = _synthetic_simulation(tmp_path, kind)
    mesh = sim.adaptive_mesh(0)
    _assert_same_mesh(mesh, want)
    _assert_table_rules(mesh)
    assert len(np.unique(mesh["cell_density"])) == len(mesh["cell_density"])  # (an equal density means the same leaf)
    if kind == "chain":
        assert A.leaf_levels(mesh).max() == 30 and len(mesh["cell_density"]) == 30 * 7 + 1
    upper = kind in A.DYADIC
    points = A.all_points(mesh, upper_walls=upper, num_random=500)
    assert A.cannot_locate(mesh, points) == []
    got = sim.imported_densities(0, points)
    assert np.array_equal(_bits(got), _bits(A.Descent(mesh).densities(points)))
    if upper:
        hi = mesh["node_box"][0, 3:]
        assert sim.imported_densities(0, hi[None, :])[0] > 0  # (the closed root box)


@pytest.mark.parametrize("name", ["cfg6amr", "cfg6amrnum", "cfg6amrelec"])
def test_cell_densities_equal_the_reference(name):
    """the tree of the spatial grid (100 densities per node) and the number density of component 0 in every cell (100 per cell), bit for bit:
    a mass density; numbers of entities with a mass fraction, metallicity and temperature cutoff; electrons as a number density, for which
    the metallicity and temperature columns are read and not used (ImportedMedium.cpp:47-57)"""
    sim = Simulation(ski(name + ".ski")).setup()
    gold = np.load(golden(name + "_cells.npz"))
    head = scene_head(sim)
    assert head.grid.num_cells == len(gold["density"])
    density = np.ctypeslib.as_array(head.medium.number_density, shape=(head.grid.num_cells,))
    assert np.array_equal(_bits(density), _bits(gold["density"]))
    assert (density > 0).sum() > 0.9 * len(density)
    assert sim.phase_functions[0] == (1 if name == "cfg6amrelec" else 0)  # (PMC_PHASE_DIPOLE for the electrons)


def test_output_files_are_the_reference_s(tmp_path):
    """the oracle's photon loop with the reference's random stream on the host layer's scene: every file of cfg6amr byte for byte"""
    sim = Simulation(ski("cfg6amr.ski")).setup()
    frames, counters = O.run_primary(sim, 0, sim.num_packets, O.RNG_MT19937)
    assert counters.histories == sim.num_packets == 20000
    sim.write(frames, str(tmp_path))
    expected = sorted(f for f in os.listdir(golden("")) if f.startswith("cfg6amr_i"))
    assert len(expected) == 11
    for f in expected:
        assert _same_file(golden(f), str(tmp_path / f)), f"{f} differs from the reference output"


def assert_convergence_files(outdir):
    """the info file and the six cut files of cfg6amrconv in outdir are the reference's"""
    name = "cfg6amrconv"
    K.assert_info_equals_golden(name, outdir)
    recorded = np.load(golden(name + "_cuts.npz"))
    files = sorted(k[len("digest/"):] for k in recorded.files if k.startswith("digest/"))
    assert files == sorted(f"{name}_cnv_dust_{kind}_{plane}.fits" for kind in "tg" for plane in ("xy", "xz", "yz"))
    assert sorted(os.listdir(outdir)) == sorted(files + [K.info_file(name)])
    for f in files:
        data = open(os.path.join(outdir, f), "rb").read()
        if K.cut_digest(data) != recorded["digest/" + f].tobytes():
            got, want = K.cut_pixels(data)[::16, ::16].astype(np.float64), recorded["pixels/" + f]
            bad = np.argwhere(got != want)
            raise AssertionError(f"{f} differs from the reference's file; {len(bad)} of {want.size} decimated pixels differ, first {bad[:1].tolist()}")


def test_convergence_info_and_cuts_are_the_reference_s(tmp_path):
    """cfg6amrconv: a mesh symmetric about the origin, so that every pixel of the three true-density cuts lies ON cell walls of the mesh, and
    Snapshot::SigmaX/Y/Z (the input optical depths of the info file) samples walls too: the wall rule against the reference itself"""
    sim = Simulation(ski("cfg6amrconv.ski")).setup()
    assert sim.dimension() == 3
    sim.write_probes(str(tmp_path), _oracle_integrator(sim), sampler=_python_sampler(sim))
    assert_convergence_files(str(tmp_path))
    # the planes of the cuts are walls of the mesh at every level: the centre of the domain is a corner of eight leaves
    mesh = sim.adaptive_mesh(0)
    boxes = A.leaf_boxes(mesh)
    assert ((boxes[:, :3] == 0.).any(axis=1) | (boxes[:, 3:] == 0.).any(axis=1)).sum() > 100
    assert (np.abs(boxes[:, :3]).max(axis=1) == 0.).sum() == 1  # (one leaf has its lower corner at the origin)


# ---------------------------------------------------------------- the six mass types on 2x2x2 cells of 1 x 1 x 2 m: volume 2 m3

ROWS = [  # density, mass, metallicity, temperature
    (4., 16., 0.5, 10.), (2., 2., 0.25, 10.), (-1., -3., 0.5, 10.), (8., 1., 0.5, 5000.),
    (0., 0., 0.5, 10.), (1., 4., 1., 10.), (0.5, 0.25, 0.5, 10.), (3., 6., 0., 10.)]
MASS_TYPES = {  # massType -> (has a density column, has a mass column)
    "MassDensity": (True, False), "Mass": (False, True), "MassDensityAndMass": (True, True),
    "NumberDensity": (True, False), "Number": (False, True), "NumberDensityAndNumber": (True, True)}
# massFraction 0.5, metallicity on, cutoff at 1000 K (cell 3 is hot, cell 2 negative): by hand, with V = 2
#   from the density column: 4*.5*.5=1, 2*.25*.5=.25, 0, 0, 0, 1*1*.5=.5, .5*.5*.5=.125, 0
#   from the mass column:    16*.5*.5=4, 2*.25*.5=.25, 0, 0, 0, 4*1*.5=2, .25*.5*.5=.0625, 0
DENSITY_FROM_DENSITY = [1., 0.25, 0., 0., 0., 0.5, 0.125, 0.]
MASS_FROM_MASS = [4., 0.25, 0., 0., 0., 2., 0.0625, 0.]


def _mass_type_simulation(tmp_path, mass_type, mix="dust"):
    has_density, has_mass = MASS_TYPES[mass_type]
    number = mass_type.startswith("Number")
    header, column = [], 1
    for present, title in ((has_density, "number density (1/m3)" if number else "mass density (kg/m3)"), (has_mass, "number (1)" if number else "mass (kg)"),
                           (True, "metallicity (1)"), (True, "temperature (K)")):
        if present:
            header.append("# column %d: %s" % (column, title))
            column += 1
    rows = [" ".join(repr(v) for v, present in zip(row, (has_density, has_mass, True, True)) if present) for row in ROWS]
    mesh = A.MeshBuilder((0., 0., 0., 2., 2., 4.))
    mesh.subdivide(0, (2, 2, 2))
    tables = A._finish(mesh)
    path = str(tmp_path / "types_mesh.txt")
    A.write_mesh_file(tables, path, header=header, rows=rows)
    replace = [('massType="MassDensity"', 'massType="%s"' % mass_type), ('massFraction="1"', 'massFraction="0.5"'),
               ('importMetallicity="false"', 'importMetallicity="true"'), ('importTemperature="false"', 'importTemperature="true"'),
               ('maxTemperature="0 K"', 'maxTemperature="1000 K"')]
    if mix == "electrons":
        text = open(ski("cfg6amr.ski")).read()
        start = text.index('<materialMix type="MaterialMix">')
        end = text.index("</materialMix>") + len("</materialMix>")
        replace.append((text[start:end], '<materialMix type="MaterialMix"><ElectronMix/></materialMix>'))
    return Simulation(A.mesh_ski(tmp_path, "types", path, (0., 0., 0., 2., 2., 4.), replace)).setup()


@pytest.mark.parametrize("mass_type", list(MASS_TYPES))
def test_mass_types_against_hand_computed_values(mass_type, tmp_path):
    """Snapshot::calculateDensityAndMass (Snapshot.cpp:325-384): the density from the density column, else from the mass over the volume; the
    mass from the mass column, else from the density times the volume; a hot cell and a negative value give zero; metallicity and mass
    fraction multiply"""
    sim = _mass_type_simulation(tmp_path, mass_type)
    has_density, has_mass = MASS_TYPES[mass_type]
    density = DENSITY_FROM_DENSITY if has_density else [m / 2. for m in MASS_FROM_MASS]
    mass = MASS_FROM_MASS if has_mass else [2. * d for d in DENSITY_FROM_DENSITY]
    assert sim.adaptive_mesh(0)["cell_density"].tolist() == density
    assert sim.imported_mass(0) == sum(mass) == (6.3125 if has_mass else 3.75)


def test_electrons_take_neither_the_temperature_cutoff_nor_the_metallicity(tmp_path):
    """ImportedMedium.cpp:53-57: the columns are read, the mass fraction applies, the hot cell counts"""
    sim = _mass_type_simulation(tmp_path, "NumberDensity", mix="electrons")
    assert sim.adaptive_mesh(0)["cell_density"].tolist() == [2., 1., 0., 4., 0., 0.5, 0.25, 1.5]
    assert sim.imported_mass(0) == 2. * 9.25
    assert sim.phase_functions[0] == 1


def test_imported_sites_are_the_leaf_centres_in_file_order():
    """VoronoiMeshSpatialGrid with the ImportedSites policy on an adaptive mesh medium: the medium offers the centres of its leaves in file
    order (AdaptiveMeshSnapshot.cpp:241-244); the grid keeps every one of them and numbers its cells by their x coordinate, as for any
    list of sites (VoronoiMeshSnapshot.cpp:494-526)"""
    sim = Simulation(ski("cfg6amrsites.ski")).setup()
    mesh = sim.adaptive_mesh(0)
    boxes = A.leaf_boxes(mesh)
    grid = scene_head(sim).grid
    assert grid.kind == K.GRID_VORONOI and grid.num_cells == len(boxes) == 2502
    sites = np.ctypeslib.as_array(grid.site, shape=(grid.num_cells, 3))
    centres = 0.5 * (boxes[:, :3] + boxes[:, 3:])
    rows = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(_bits(rows(sites)), _bits(rows(centres)))
    assert (np.diff(sites[:, 0]) >= 0).all()


# ---------------------------------------------------------------- errors, by their words

UNSUPPORTED = "ski: %s is not supported on the MI355X primary-emission path"
PAN = ('simulationMode="OligoExtinctionOnly"', 'simulationMode="ExtinctionOnly"')
ELECTRONS = '<materialMix type="MaterialMix"><ElectronMix/></materialMix>'


def _refusal(tmp_path, replace, mesh_text=None, extent_m=None):
    path = ski("cfg6amr_mesh.txt")
    if mesh_text is not None:
        path = str(tmp_path / "broken_mesh.txt")
        with open(path, "w") as fh:
            fh.write(mesh_text)
    try:
        Simulation(A.mesh_ski(tmp_path, "broken", path, extent_m, replace)).setup()
    except RuntimeError as error:
        return str(error)
    return None


@pytest.mark.parametrize("replace,message", [
    ([PAN, ('importVelocity="false"', 'importVelocity="true"')], UNSUPPORTED % "an imported medium with a velocity field"),
    ([('importMagneticField="false"', 'importMagneticField="true"')], UNSUPPORTED % "an imported medium with a magnetic field"),
    ([('importVariableMixParams="false"', 'importVariableMixParams="true"')], UNSUPPORTED % "an imported medium with a variable material mix"),
    ([('useColumns=""', 'useColumns="x, y"')], UNSUPPORTED % "useColumns (column remapping)"),
    ([('maxX="17000 pc"', 'maxX="-19000 pc"')], "The extent of the domain should be positive in the X direction"),
    ([('maxY="18300 pc"', 'maxY="-16501 pc"')], "The extent of the domain should be positive in the Y direction"),
    ([('minZ="-3700 pc"', 'minZ="3100 pc"')], "The extent of the domain should be positive in the Z direction"),
    ([('massType="MassDensity"', 'massType="Weight"')], UNSUPPORTED % "massType Weight"),
    ([('AdaptiveMeshMedium', 'CellMedium')], UNSUPPORTED % "medium CellMedium"),
])
def test_the_reader_refuses_in_these_words(tmp_path, replace, message):
    assert _refusal(tmp_path, replace) == message


def test_a_missing_filename(tmp_path):
    text = open(ski("cfg6amr.ski")).read().replace(' filename="cfg6amr_mesh.txt"', "")
    (tmp_path / "nofile.ski").write_text(text)
    with pytest.raises(RuntimeError, match="^ski: AdaptiveMeshMedium lacks a filename$"):
        Simulation(str(tmp_path / "nofile.ski"))


def test_importing_a_velocity_is_ignored_in_an_oligochromatic_simulation(tmp_path):
    assert _refusal(tmp_path, [('importVelocity="false"', 'importVelocity="true"')]) is None


def test_electrons_stay_refused_in_a_particle_medium_and_pass_in_a_mesh(tmp_path):
    text = open(ski("cfg4small.ski")).read()
    start, end = text.index('<materialMix type="MaterialMix">'), text.index("</materialMix>") + len("</materialMix>")
    (tmp_path / "cfg4small.ski").write_text(text[:start] + ELECTRONS + text[end:])
    with pytest.raises(RuntimeError, match="ElectronMix in a ParticleMedium"):
        Simulation(str(tmp_path / "cfg4small.ski"))
    Simulation(ski("cfg6amrelec.ski"))


TWO = "! 2 1 1\n"


@pytest.mark.parametrize("mesh_text,message", [
    ("! 2 2\n1\n1\n1\n1\n", "Nonleaf subdivision specifiers are missing or not formatted as integers"),
    ("! 2 x 1\n1\n1\n", "Nonleaf subdivision specifiers are missing or not formatted as integers"),
    (TWO + "1\n", "Reached end of file in adaptive mesh data before all nodes were read"),
    (TWO + "! 1 1 2\n1\n# a comment\n\n", "Reached end of file in adaptive mesh data before all nodes were read"),
    (TWO + "1\n2\n3\n", "Superfluous lines in adaptive mesh data after all nodes were read"),
    ("1\n\n# note\n  2\n", "Superfluous lines in adaptive mesh data after all nodes were read"),
    (TWO + "1\nabc\n", "Input text is not formatted as a floating point number: abc"),
    ("# column 1: mass density (kg/m3)\n" + TWO + "1\n2\n", None),
    ("# column 1: mass density (furlongs)\n" + TWO + "1\n2\n", "Invalid units (furlongs) for quantity 'massvolumedensity' in column 1"),
    ("# column 2: mass density (kg/m3)\n" + TWO + "1\n2\n", "Incorrect column index in file header for column 1"),
    ("! 0 1 1\n", "Nonleaf subdivision specifiers should be positive"),
])
def test_the_file_fails_in_these_words(tmp_path, mesh_text, message):
    assert _refusal(tmp_path, [], mesh_text) == message


def test_comments_and_blank_lines_are_skipped_anywhere(tmp_path):
    text = "# head\n\n  # column 1: mass density (kg/m3)\n\n" + "! 2 1 1\n# between\n\n 0.5\n   \n! 1 1 2  \n#x\n0.25\n\n0.125 # trailing words\n\n# tail\n"
    path = tmp_path / "comments_mesh.txt"
    path.write_text(text)
    sim = Simulation(A.mesh_ski(tmp_path, "comments", str(path), (0., 0., 0., 2., 1., 1.))).setup()
    mesh = sim.adaptive_mesh(0)
    assert mesh["cell_density"].tolist() == [0.5, 0.25, 0.125] and mesh["node_dims"].tolist() == [[2, 1, 1], [0, 0, 0], [1, 1, 2], [0, 0, 0], [0, 0, 0]]
    assert mesh["node_link"].tolist() == [1, 0, 3, 1, 2]
    assert mesh["node_box"][4].tolist() == [1., 0., 0.5, 2., 1., 1.]
    assert sim.imported_densities(0, [[0.5, 0.5, 0.5], [1.5, 0.5, 0.25], [1.5, 0.5, 0.75], [1., 0.5, 0.5], [2.5, 0.5, 0.5]]).tolist() == [0.5, 0.25, 0.125, 0.125, 0.]


def test_a_position_in_a_rounding_gap_fails_in_the_reference_s_words(tmp_path):
    """Where lo + 3 * (hi - lo) / 3 rounds below hi, the upper wall of the root lies in no child: the index correction of Node::child leaves
    the child list (the reference reads outside it there), which is the reference's error here -- for the single position on the host, and
    with the lowest failing index for a batch"""
    rng = np.random.default_rng(5)
    lo, hi = next((a, b) for a, b in zip(rng.random(1000), 1. + rng.random(1000)) if A.frac_pos(a, b, 3, 3) < b)
    path = tmp_path / "gap_mesh.txt"
    path.write_text("# column 1: mass density (kg/m3)\n! 3 1 1\n1\n2\n3\n")
    sim = Simulation(A.mesh_ski(tmp_path, "gap", str(path), (lo, 0., 0., hi, 1., 1.))).setup()
    mesh = sim.adaptive_mesh(0)
    assert mesh["node_box"][3, 3] < hi == mesh["node_box"][0, 3]
    inside = [0.5 * (lo + hi), 0.5, 0.5]
    assert A.cannot_locate(mesh, [inside, [hi, 0.5, 0.5]]) == [1]
    assert sim.imported_densities(0, [inside]).tolist() == [2.]
    with pytest.raises(RuntimeError, match=r"^Can't locate the appropriate child node \(position 2\)$"):
        sim.imported_densities(0, [inside, inside, [hi, 0.5, 0.5], inside, [hi, 0.25, 0.5]])


def test_a_component_of_another_kind_has_no_mesh():
    sim = Simulation(ski("cfg4small.ski")).setup()
    with pytest.raises(RuntimeError, match="is a ParticleMedium, not an AdaptiveMeshMedium"):
        sim.adaptive_mesh(0)
    assert sim.imported_densities(0, [[0., 0., 0.]])[0] > 0  # (the particle snapshot answers the same call)
    with pytest.raises(RuntimeError, match="not an imported medium"):
        Simulation(ski("cfg2small.ski")).setup().imported_densities(0, [[0., 0., 0.]])
    with pytest.raises(RuntimeError, match="no such medium component"):
        sim.imported_mass(3)


# the scene files of the particle scenes as the parent of this change wrote them (sha256): the shared ImportedMedium base changes nothing
PARTICLE_SCENES = {"cfg4small": "10402be460fc3652c932fc29f05e9e75388de1252feec5ef5f9e05d3c19139d3",
                   "cfg5imp": "8b9c913a6df1150944e46c43040a419f9b67261001aabe218d48df1f20ac68b5"}


@pytest.mark.parametrize("name", list(PARTICLE_SCENES))
def test_particle_scene_files_are_unchanged(name, tmp_path):
    Simulation(ski(name + ".ski")).setup().save_scene(str(tmp_path / "scene.bin"))
    assert hashlib.sha256(open(tmp_path / "scene.bin", "rb").read()).hexdigest() == PARTICLE_SCENES[name]
