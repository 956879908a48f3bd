"""What the ski reader (skirt9_amd/host/ski_reader.cpp) and Simulation::setup refuse, and in which words: one table of (fixture, edits, message).
Every row takes a small fixture of tests/ski, makes one change to it (a change may take several replacements: a renamed element has two tags) and
expects the text of one refusal site.  The texts are literals, recorded from the build before the reader was split into its functions: they do
not come from the code under test.  The rows of ORDER carry two defects each and pin which of them is named: the order of the checks.  No GPU."""
import re

import pytest

from conftest import ski
from skirt9_amd.host import Simulation

UNSUPPORTED = "ski: %s is not supported on the MI355X primary-emission path"

# ---- pieces of the fixtures that the edits replace
C1_BOX = '<UniformBoxGeometry minX="-1 pc" maxX="1 pc" minY="-1 pc" maxY="1 pc" minZ="-1 pc" maxZ="1 pc"/>'
C1_MESHX = '<LinMesh numBins="32"/></meshX>'
C1_NORM = '<OpticalDepthMaterialNormalization axis="X" wavelength="0.55 micron" opticalDepth="2"/>'
C1_LUM = '<IntegratedLuminosityNormalization wavelengthRange="Source" integratedLuminosity="1 Lsun"/>'
C1_LOGGRID = '<LogWavelengthGrid minWavelength="0.1 micron" maxWavelength="1 micron" numWavelengths="2"/>'
C1_MEDIUM = '<GeometricMedium velocityMagnitude="0 km/s" magneticFieldStrength="0 uG">'
NO_PROBES = '<probeSystem type="ProbeSystem"><ProbeSystem/></probeSystem>'
T_BOX = '<UniformBoxGeometry minX="-1.5 pc" maxX="0.5 pc" minY="-0.7 pc" maxY="0.9 pc" minZ="-0.25 pc" maxZ="0.25 pc"/>'
T_BIAS = '<LogWavelengthDistribution minWavelength="0.1 micron" maxWavelength="10 micron"/>'
T_TC = '<TemperatureProbe probeName="tc" probeAfter="Run" aggregation="Type">'
T_RF = '<RadiationFieldProbe probeName="rf" writeWavelengthGrid="false" probeAfter="Run">'
K_FIELD = '<CylindricalVectorField unityRadius="2000 pc" exponent="1"/>'
K_SED = 'wavelengths="0.5495 micron, 0.55 micron, 0.5505 micron" specificLuminosities="0.001 W/micron, 1 W/micron, 0.001 W/micron"'
GAUSS = '<GaussianGeometry dispersion="1 pc"/>'
OWN_GRID = ('<wavelengthGrid type="WavelengthGrid"><LogWavelengthGrid minWavelength="0.2 micron" maxWavelength="2 micron" numWavelengths="3"/>'
            '</wavelengthGrid>')
RF_ON = ('storeRadiationField="true"><radiationFieldWLG type="DisjointWavelengthGrid"><LogWavelengthGrid minWavelength="0.5 micron" '
         'maxWavelength="0.6 micron" numWavelengths="3"/></radiationFieldWLG></RadiationFieldOptions>')
DEFAULT_GRID = re.compile(r"<defaultWavelengthGrid.*?</defaultWavelengthGrid>", re.S)
ONE_MEDIUM = re.compile(r"(<GeometricMedium.*</GeometricMedium>)", re.S)


def inside(geometry, decorator):
    return '<%s><geometry type="Geometry">%s</geometry></%s>' % (decorator, geometry, decorator.split()[0])


def probes(text):
    return '<probeSystem type="ProbeSystem"><ProbeSystem><probes type="Probe">' + text + "</probes></ProbeSystem></probeSystem>"


def renamed(old, new):
    """an element under another name: its start tag (which has attributes or children) and its end tag"""
    return [("<" + old + " ", "<" + new + " "), ("</" + old + ">", "</" + new + ">")]


def removed(pattern):
    return [(re.compile(pattern, re.S), "")]


PAN = [('simulationMode="OligoExtinctionOnly"', 'simulationMode="ExtinctionOnly"')]

# (fixture, [(old, new), ...], message): old is a string or a compiled pattern, replaced once
ROWS = [
    # ---- attribute access, geometries, wavelength grids
    ("cfg1.ski", [(' opticalDepth="2"', "")], "ski: <OpticalDepthMaterialNormalization> lacks the required attribute 'opticalDepth'"),
    ("cfg1.ski", [('recordStatistics="true"', 'recordStatistics="maybe"')], "ski: invalid boolean 'maybe' for attribute recordStatistics"),
    ("cfg1.ski", [(C1_BOX, "<OffsetGeometryDecorator/>")], "ski: OffsetGeometryDecorator lacks a geometry"),
    ("cfg1.ski", [(C1_BOX, '<SpheroidalGeometryDecorator flattening="0.5"/>')], "ski: SpheroidalGeometryDecorator lacks a geometry"),
    ("cfg1.ski", [(C1_BOX, inside(C1_BOX, 'SpheroidalGeometryDecorator flattening="0.5"'))], UNSUPPORTED % "SpheroidalGeometryDecorator of UniformBoxGeometry"),
    ("cfg1.ski", [(C1_BOX, "<ConicalShellGeometry/>")], UNSUPPORTED % "geometry ConicalShellGeometry"),
    ("cfg1.ski", [('maxWavelength="1 micron" numWavelengths="2"', 'maxWavelength="0.05 micron" numWavelengths="2"')], "the longest wavelength should be larger than the shortest"),
    ("cfg3kin.ski", [('maxWavelength="0.57 micron"', 'maxWavelength="0.5 micron"')], "the longest wavelength should be larger than the shortest"),
    ("cfg1.ski", [(C1_LOGGRID, "<NestedLogWavelengthGrid/>")], UNSUPPORTED % "wavelength grid NestedLogWavelengthGrid"),
    # ---- root, units, mode, random, cosmology
    ("cfg1.ski", [('<skirt-simulation-hierarchy type="MonteCarloSimulation"', '<skirt-simulation-hierarchy type="Other"')], "ski: the root element is not a skirt-simulation-hierarchy of type MonteCarloSimulation"),
    ("cfg1.ski", renamed("MonteCarloSimulation", "OtherSimulation"), "ski: missing MonteCarloSimulation element"),
    ("cfg1.ski", [('<ExtragalacticUnits wavelengthOutputStyle="Wavelength" fluxOutputStyle="Frequency"/>', "<ImperialUnits/>")], UNSUPPORTED % "unit system ImperialUnits"),
    ("cfg1.ski", [('wavelengthOutputStyle="Wavelength"', 'wavelengthOutputStyle="Frequency"')], UNSUPPORTED % "wavelengthOutputStyle Frequency"),
    ("cfg1.ski", [('fluxOutputStyle="Frequency"', 'fluxOutputStyle="Energy"')], UNSUPPORTED % "fluxOutputStyle Energy"),
    ("cfg1.ski", [('simulationMode="OligoExtinctionOnly"', 'simulationMode="DustEmission"')], UNSUPPORTED % "simulationMode DustEmission"),
    ("cfg1.ski", [('numPackets="1e6">', 'numPackets="1e6" iteratePrimaryEmission="true">')], UNSUPPORTED % "iteratePrimaryEmission"),
    ("cfg1.ski", [('<Random seed="0"/>', '<FastRandom seed="0"/>')], UNSUPPORTED % "random generator FastRandom"),
    ("cfg3z.ski", [('redshift="0.5"', 'redshift="0"')], UNSUPPORTED % "FlatUniverseCosmology with redshift zero"),
    ("cfg1.ski", [("<LocalUniverseCosmology/>", "<SteadyStateCosmology/>")], UNSUPPORTED % "cosmology SteadyStateCosmology"),
    # ---- source system
    ("cfg1.ski", renamed("sourceSystem", "sourcesSystem"), "ski: missing sourceSystem"),
    ("cfg1.ski", removed(r"<PointSource.*</PointSource>"), UNSUPPORTED % "a source system with 0 sources"),
    ("cfg1laser.ski", [('symmetryX="0" symmetryY="-1" symmetryZ="0.2"', 'symmetryX="0" symmetryY="0" symmetryZ="0"')], "Symmetry axis direction cannot be null vector"),
    ("cfg1.ski", [("<IsotropicAngularDistribution/>", "<DiskAngularDistribution/>")], UNSUPPORTED % "angular distribution DiskAngularDistribution"),
    ("cfg1.ski", [("<NoPolarizationProfile/>", "<LinearPolarizationProfile/>")], UNSUPPORTED % "polarization profile LinearPolarizationProfile"),
    ("cfg1temp.ski", removed(r'<geometry type="Geometry"><UniformBoxGeometry minX="-1.5 pc".*?</geometry>'), "ski: GeometricSource lacks a geometry"),
    ("cfg1temp.ski", [(T_BOX, GAUSS)], UNSUPPORTED % "source geometry GaussianGeometry"),
    ("cfg1temp.ski", [(T_BOX, inside(GAUSS, 'OffsetGeometryDecorator offsetX="1 pc"'))], UNSUPPORTED % "source geometry GaussianGeometry"),
    ("cfg1temp.ski", [(T_BOX, inside(GAUSS, 'SpheroidalGeometryDecorator flattening="0.5"'))], UNSUPPORTED % "source geometry SpheroidalGeometryDecorator of GaussianGeometry"),
    ("cfg3kin.ski", [(K_FIELD, '<OffsetVectorFieldDecorator offsetX="1 pc"/>')], "ski: OffsetVectorFieldDecorator lacks a vectorField"),
    ("cfg3kin.ski", [(K_FIELD, '<UnidirectionalVectorField fieldX="0" fieldY="0" fieldZ="0"/>')], "Field direction cannot be null vector"),
    ("cfg3kin.ski", [(K_FIELD, "<HollowRadialVectorField/>")], UNSUPPORTED % "vector field HollowRadialVectorField"),
    ("cfg1.ski", renamed("PointSource", "CubicalBackgroundSource"), UNSUPPORTED % "source CubicalBackgroundSource"),
    ("cfg3kin.ski", [('<ListSED unitStyle="wavelengthmonluminosity"', '<ListSED unitStyle="frequencymonluminosity"')], UNSUPPORTED % "ListSED unitStyle frequencymonluminosity"),
    ("cfg3kin.ski", [('specificLuminosities="0.001 W/micron, 1 W/micron, 0.001 W/micron"', 'specificLuminosities="0.001 W/micron, 1 W/micron"')], "Number of listed luminosities does not match number of listed wavelengths"),
    ("cfg3sed.ski", [('<FileSED filename="cfg3sed_sed.txt"/>', "<FileSED/>")], "ski: FileSED lacks a filename"),
    ("cfg1.ski", [('<BlackBodySED temperature="5000 K"/>', "<SunSED/>")], UNSUPPORTED % "SED SunSED"),
    ("cfg3kin.ski", [(K_SED, 'wavelengths="0.55 micron" specificLuminosities="1 W/micron"')], "SED must have at least two wavelength/luminosity pairs"),
    ("cfg3norm.ski", [('unitStyle="frequencymonluminosity"', 'unitStyle="energymonluminosity"')], UNSUPPORTED % "SpecificLuminosityNormalization unitStyle energymonluminosity"),
    ("cfg1.ski", [(C1_LUM, "<BandLuminosityNormalization/>")], UNSUPPORTED % "luminosity normalization BandLuminosityNormalization"),
    ("cfg1.ski", removed(r'<normalization type="LuminosityNormalization">.*?</normalization>'), "ski: source lacks a luminosity normalization"),
    ("cfg1temp.ski", [(T_BIAS, "<DiscreteWavelengthDistribution/>")], UNSUPPORTED % "wavelength bias distribution DiscreteWavelengthDistribution"),
    # ---- medium system
    ("cfg1.ski", renamed("mediumSystem", "mediaSystem"), "ski: simulationMode OligoExtinctionOnly needs a medium system"),
    ("cfg1temp.ski", [('forceScattering="true"', 'forceScattering="false"')], UNSUPPORTED % "storeRadiationField without forceScattering"),
    ("cfg1temp.ski", removed(r"<radiationFieldWLG.*?</radiationFieldWLG>"), "ski: RadiationFieldOptions lacks a radiationFieldWLG"),
    ("cfg1.ski", [(ONE_MEDIUM, "")], UNSUPPORTED % "a medium system without media"),
    ("cfg1.ski", [(ONE_MEDIUM, r"\1\1\1\1\1")], UNSUPPORTED % "a medium system with more than 4 media"),
    ("cfg3kin.ski", [(ONE_MEDIUM, r"\1\1")], UNSUPPORTED % "a moving source together with more than one medium component"),
    ("cfg3kin.ski", [('storeRadiationField="false"/>', RF_ON)], UNSUPPORTED % "a moving source together with storeRadiationField"),
    ("cfg1.ski", renamed("GeometricMedium", "CellMedium"), UNSUPPORTED % "medium CellMedium"),
    ("cfg1temp.ski", [(C1_MEDIUM, '<GeometricMedium velocityMagnitude="100 km/s" magneticFieldStrength="0 uG">'
                       '<velocityDistribution type="VectorField"><RadialVectorField/></velocityDistribution>')], UNSUPPORTED % "a medium with a velocity field"),
    ("cfg1.ski", [(C1_MEDIUM, '<GeometricMedium velocityMagnitude="0 km/s" magneticFieldStrength="1 uG">'
                   '<magneticFieldDistribution type="VectorField"><RadialVectorField/></magneticFieldDistribution>')], UNSUPPORTED % "a medium with a magnetic field"),
    ("cfg1.ski", removed(r"<materialMix.*?</materialMix>"), "ski: GeometricMedium lacks a material mix"),
    ("cfg1.ski", [(re.compile(r"<MeanListDustMix[^>]*/>"), "<ZubkoDustMix/>")], UNSUPPORTED % "material mix ZubkoDustMix"),
    ("cfg1elec.ski", [('includePolarization="false"', 'includePolarization="true"')], UNSUPPORTED % "ElectronMix with includePolarization"),
    ("cfg1elec.ski", PAN + [('includeThermalDispersion="false"', 'includeThermalDispersion="true"')], UNSUPPORTED % "ElectronMix with includeThermalDispersion in a panchromatic simulation"),
    ("cfg4small.ski", [(re.compile(r'(<materialMix type="MaterialMix">).*?(</materialMix>)', re.S), r"\1<ElectronMix/>\2")], UNSUPPORTED % "ElectronMix in a ParticleMedium"),
    ("cfg1file.ski", [('<MeanFileDustMix filename="cfg1file_dust.txt"/>', "<MeanFileDustMix/>")], "ski: MeanFileDustMix lacks a filename"),
    ("cfg1.ski", removed(r'<geometry type="Geometry"><UniformBoxGeometry.*?</geometry>'), "ski: GeometricMedium lacks a geometry"),
    ("cfg1.ski", removed(r'<normalization type="MaterialNormalization">.*?</normalization>'), "ski: GeometricMedium lacks a normalization"),
    ("cfg1.ski", [(C1_NORM, "<MassColumnMaterialNormalization/>")], UNSUPPORTED % "material normalization MassColumnMaterialNormalization"),
    ("cfg4small.ski", [(' filename="cfg4small_sph.txt"', "")], "ski: ParticleMedium lacks a filename"),
    ("cfg4small.ski", [('massType="Mass"', 'massType="Volume"')], UNSUPPORTED % "massType Volume"),
    ("cfg4small.ski", PAN + [('importVelocity="false"', 'importVelocity="true"')], UNSUPPORTED % "an imported medium with a velocity field"),
    ("cfg4small.ski", [('importMagneticField="false"', 'importMagneticField="true"')], UNSUPPORTED % "an imported medium with a magnetic field"),
    ("cfg4small.ski", [('importVariableMixParams="false"', 'importVariableMixParams="true"')], UNSUPPORTED % "an imported medium with a variable material mix"),
    ("cfg4small.ski", [('useColumns=""', 'useColumns="x, y"')], UNSUPPORTED % "useColumns (column remapping)"),
    # ---- spatial grid
    ("cfg1.ski", removed(r'<grid type="SpatialGrid">.*</grid>'), "ski: MediumSystem lacks a spatial grid"),
    ("cfg1.ski", [(C1_MESHX, '<ListMesh points=""/></meshX>')], "The mesh data file has no points"),
    ("cfg1.ski", [(C1_MESHX, '<ListMesh points="-1, 2"/></meshX>')], "The mesh data file has negative points"),
    ("cfg1.ski", [(C1_MESHX, '<ListMesh points="0"/></meshX>')], "The mesh data file has no positive points"),
    ("cfg1.ski", [(C1_MESHX, "<FileMesh/></meshX>")], UNSUPPORTED % "mesh FileMesh"),
    ("cfg1.ski", [(C1_MESHX, '<LinMesh numBins="30000"/></meshX>')], UNSUPPORTED % "a Cartesian grid with more than 20000 bins on its three axes together, or 2^31 cells"),
    ("cfg2small.ski", [('treeType="OctTree"', 'treeType="HexTree"')], UNSUPPORTED % "treeType HexTree"),
    ("cfg2small.ski", [(re.compile(r"<DensityTreePolicy[^>]*/>"), "<SiteListTreePolicy/>")], UNSUPPORTED % "tree policy SiteListTreePolicy"),
    ("cfg5small.ski", [('policy="Uniform"', 'policy="Lloyd"')], UNSUPPORTED % "Voronoi site policy Lloyd"),
    ("cfg5small.ski", [('policy="Uniform"', 'policy="File"')], "ski: VoronoiMeshSpatialGrid lacks a filename"),
    ("cfg1.ski", renamed("CartesianSpatialGrid", "Cylinder2DSpatialGrid"), UNSUPPORTED % "spatial grid Cylinder2DSpatialGrid"),
    # ---- instrument system
    ("cfg1.ski", renamed("instrumentSystem", "instrumentsSystem"), "ski: missing instrumentSystem"),
    ("cfg1.ski", [("<FullInstrument instrumentName", "<AllSkyInstrument instrumentName")], UNSUPPORTED % "instrument AllSkyInstrument"),
    ("cfg1.ski", [('recordPolarization="false"', 'recordPolarization="true"')], UNSUPPORTED % "recordPolarization"),
    ("cfg1.ski", [('distance="1 Mpc"', 'distance="0 Mpc"')], "Instrument distance and model redshift are both zero"),
    ("cfg1.ski", removed(r"<FullInstrument[^>]*/>"), UNSUPPORTED % "a simulation without instruments"),
    # ---- probe system
    ("cfg1.ski", [(NO_PROBES, probes('<TemperatureProbe probeName="t"><form type="Form"><PerCellForm/></form></TemperatureProbe>'))], UNSUPPORTED % "TemperatureProbe in an oligochromatic simulation"),
    ("cfg1temp.ski", [('storeRadiationField="true"', 'storeRadiationField="false"')], UNSUPPORTED % "TemperatureProbe in a simulation that does not store the radiation field"),
    ("cfg1temp.ski", [('probeName="ab" writeWavelengthGrid="false"', 'probeName="ab" writeWavelengthGrid="true"')], UNSUPPORTED % "DustAbsorptionPerCellProbe writeWavelengthGrid"),
    ("cfg1temp.ski", [(T_TC + '<form type="Form"><PerCellForm/>', T_TC + '<form type="Form"><LinearCutForm/>')], UNSUPPORTED % "TemperatureProbe form LinearCutForm"),
    ("cfg1probe.ski", [('aggregation="Type"><form type="Form"><PerCellForm/>', 'aggregation="Type"><form type="Form"><LinearCutForm/>')], UNSUPPORTED % "probe form LinearCutForm"),
    ("cfg1probe.ski", removed(r'<form type="Form"><PerCellForm/></form>'), UNSUPPORTED % "probe form DefaultCutsForm"),
    ("cfg1temp.ski", [(T_TC, T_TC.replace('probeAfter="Run"', 'probeAfter="Setup"'))], UNSUPPORTED % "TemperatureProbe probeAfter Setup"),
    ("cfg1probe.ski", [('probeName="dns" probeAfter="Setup"', 'probeName="dns" probeAfter="Primary"')], UNSUPPORTED % "DensityProbe probeAfter Primary"),
    ("cfg1probe.ski", [('probeName="dns" probeAfter="Setup" aggregation="Type"', 'probeName="dns" probeAfter="Setup" aggregation="Fragment"')], UNSUPPORTED % "DensityProbe aggregation Fragment"),
    ("cfg1temp.ski", [(T_TC, T_TC.replace('aggregation="Type"', 'aggregation="System"'))], "ski: invalid aggregation 'System' for TemperatureProbe"),
    ("cfg1temp.ski", [('numPixelsY="12" centerY="0 pc" numSampling="1"', 'numPixelsY="12" centerY="0 pc" numSampling="12"')], "ski: ParallelProjectionForm of probe tf: value out of range"),
    ("cfg1temp.ski", [(T_TC, T_TC + OWN_GRID)], "ski: TemperatureProbe has no wavelengthGrid"),
    ("cfg1.ski", [(NO_PROBES, probes('<OpacityProbe probeName="o" aggregation="System"><form type="Form"><PerCellForm/></form>' + OWN_GRID
                                     + "</OpacityProbe>"))], UNSUPPORTED % "OpacityProbe wavelengthGrid in an oligochromatic simulation"),
    ("cfg1.ski", [(NO_PROBES, probes('<LuminosityProbe probeName="x"/>'))], UNSUPPORTED % "probe LuminosityProbe"),
    ("cfg1temp.ski", [(T_RF + '<form type="Form"><PerCellForm/>', T_RF + '<form type="Form"><DefaultCutsForm/>')], UNSUPPORTED % "probe form DefaultCutsForm"),
    ("cfg1temp.ski", removed(r'(?<=probeAfter="Run">)<form type="Form"><PerCellForm/></form>(?=</RadiationFieldProbe>)'), UNSUPPORTED % "probe form (none)"),
    ("cfg1temp.ski", [(T_RF, T_RF.replace('writeWavelengthGrid="false"', 'writeWavelengthGrid="true"'))], UNSUPPORTED % "RadiationFieldProbe writeWavelengthGrid"),
    ("cfg1temp.ski", [(T_RF, T_RF.replace('probeAfter="Run"', 'probeAfter="Secondary"'))], UNSUPPORTED % "RadiationFieldProbe probeAfter Secondary"),
    # ---- setup(): grids in effect, wavelength range, sources, scene
    ("cfg1temp.ski", [(DEFAULT_GRID, "")], "Cannot find a wavelength grid for instrument or probe"),
    ("cfg1temp.ski", [(DEFAULT_GRID, ""), ('recordStatistics="true"/></instruments>', 'recordStatistics="true">' + OWN_GRID + "</FrameInstrument></instruments>"),
                      (T_RF, '<OpacityProbe probeName="o" aggregation="System"><form type="Form"><PerCellForm/></form></OpacityProbe>' + T_RF)], "Cannot find a wavelength grid for instrument or probe"),
    ("cfg1elec.ski", [('<SourceSystem wavelengths="0.55 micron"', '<SourceSystem wavelengths="0.005 micron"')], UNSUPPORTED % "ElectronMix with a source or instrument wavelength below 10 nm (Compton scattering)"),
    ("cfg3kin.ski", [('minWavelength="0.54 micron" maxWavelength="0.56 micron"', 'minWavelength="0.6 micron" maxWavelength="0.7 micron"')], "Intrinsic SED wavelength range does not overlap source wavelength range"),
    ("cfg3norm.ski", [('<SpecificLuminosityNormalization wavelength="0.8 micron"', '<SpecificLuminosityNormalization wavelength="800 micron"')], "The normalization wavelength is outside of the SED's wavelength range"),
    ("cfg1temp.ski", [('wavelengthRange="Source"', 'wavelengthRange="Custom" minWavelength="2 micron" maxWavelength="1 micron"')], "the normalization wavelength range is empty"),
    ("cfg3kin.ski", [('wavelengthRange="Source"', 'wavelengthRange="Custom" minWavelength="1 micron" maxWavelength="2 micron"')], "the normalization luminosity is zero"),
    ("cfg1temp.ski", [(T_BIAS, '<LogWavelengthDistribution minWavelength="20 micron" maxWavelength="30 micron"/>')], "Wavelength distribution range does not overlap source wavelength range"),
    ("cfg1.ski", [('integratedLuminosity="1 Lsun"', 'integratedLuminosity="0 Lsun"')], "The total luminosity of the source system is zero"),
    ("cfg1.ski", [('inclination="60 deg"', 'inclination="200 deg"')], "Theta should be between 0 and pi."),
]

# two defects each, the one that stands first in the order of the checks is named
ORDER = [
    # a moving source with two media and an unknown instrument: the media
    ("cfg3kin.ski", [(ONE_MEDIUM, r"\1\1"), (re.compile(r'<FullInstrument (instrumentName="edge".*?)></FullInstrument>'), r"<AllSkyInstrument \1></AllSkyInstrument>")],
     UNSUPPORTED % "a moving source together with more than one medium component"),
    # a moving source that stores the radiation field, and an unknown medium: the cross-checks stand ahead of the media loop
    ("cfg3kin.ski", [('storeRadiationField="false"/>', RF_ON)] + renamed("GeometricMedium", "CellMedium"), UNSUPPORTED % "a moving source together with storeRadiationField"),
    # the number of media before the moving source
    ("cfg3kin.ski", [(ONE_MEDIUM, r"\1\1\1\1\1")], UNSUPPORTED % "a medium system with more than 4 media"),
    # recordPolarization stands after the instrument's other attributes, ahead of the distance
    ("cfg1.ski", [('recordPolarization="false"', 'recordPolarization="true"'), ('distance="1 Mpc"', 'distance="0 Mpc"')], UNSUPPORTED % "recordPolarization"),
    ("cfg1.ski", [('recordPolarization="false"', 'recordPolarization="true"'), ('recordStatistics="true"', 'recordStatistics="maybe"')], "ski: invalid boolean 'maybe' for attribute recordStatistics"),
    # instruments before probes, media before the grid, sources before media, units before the mode
    ("cfg1.ski", [("<FullInstrument instrumentName", "<AllSkyInstrument instrumentName"), (NO_PROBES, probes('<LuminosityProbe probeName="x"/>'))], UNSUPPORTED % "instrument AllSkyInstrument"),
    ("cfg1.ski", [(C1_MESHX, "<FileMesh/></meshX>"), (C1_NORM, "<MassColumnMaterialNormalization/>")], UNSUPPORTED % "material normalization MassColumnMaterialNormalization"),
    ("cfg1.ski", [(C1_LUM, "<BandLuminosityNormalization/>"), (C1_NORM, "<MassColumnMaterialNormalization/>")], UNSUPPORTED % "luminosity normalization BandLuminosityNormalization"),
    ("cfg1.ski", [('<ExtragalacticUnits wavelengthOutputStyle="Wavelength" fluxOutputStyle="Frequency"/>', "<ImperialUnits/>"),
                  ('simulationMode="OligoExtinctionOnly"', 'simulationMode="DustEmission"')], UNSUPPORTED % "unit system ImperialUnits"),
    # within a source: its kind, the SED, the normalisation; within a medium: the mix before the geometry
    ("cfg1.ski", [('<BlackBodySED temperature="5000 K"/>', "<SunSED/>")] + removed(r'<normalization type="LuminosityNormalization">.*?</normalization>'), UNSUPPORTED % "SED SunSED"),
    ("cfg1.ski", [("<IsotropicAngularDistribution/>", "<DiskAngularDistribution/>"), ('<BlackBodySED temperature="5000 K"/>', "<SunSED/>")], UNSUPPORTED % "angular distribution DiskAngularDistribution"),
    ("cfg1.ski", [(re.compile(r"<MeanListDustMix[^>]*/>"), "<ZubkoDustMix/>")] + removed(r'<geometry type="Geometry"><UniformBoxGeometry.*?</geometry>'), UNSUPPORTED % "material mix ZubkoDustMix"),
    ("cfg1.ski", [(C1_MEDIUM, '<GeometricMedium velocityMagnitude="0 km/s" magneticFieldStrength="1 uG">'
                   '<magneticFieldDistribution type="VectorField"><RadialVectorField/></magneticFieldDistribution>'),
                  (re.compile(r"<MeanListDustMix[^>]*/>"), "<ZubkoDustMix/>")], UNSUPPORTED % "a medium with a magnetic field"),
    # a probe that needs the radiation field says so before its form is looked at
    ("cfg1temp.ski", [('storeRadiationField="true"', 'storeRadiationField="false"'), (T_TC + '<form type="Form"><PerCellForm/>', T_TC + '<form type="Form"><LinearCutForm/>')], UNSUPPORTED % "TemperatureProbe in a simulation that does not store the radiation field"),
    # setup(): the grids in effect, then the Compton refusal, then the scene's instruments, then the source tables, then the source system
    ("cfg1temp.ski", [(DEFAULT_GRID, ""), (T_BIAS, '<LogWavelengthDistribution minWavelength="20 micron" maxWavelength="30 micron"/>')], "Cannot find a wavelength grid for instrument or probe"),
    ("cfg1elec.ski", [('<SourceSystem wavelengths="0.55 micron"', '<SourceSystem wavelengths="0.005 micron"'), ('inclination="30 deg"', 'inclination="200 deg"')], UNSUPPORTED % "ElectronMix with a source or instrument wavelength below 10 nm (Compton scattering)"),
    ("cfg1.ski", [('inclination="60 deg"', 'inclination="200 deg"'), ('integratedLuminosity="1 Lsun"', 'integratedLuminosity="0 Lsun"')], "Theta should be between 0 and pi."),
    ("cfg1temp.ski", [('inclination="35 deg"', 'inclination="200 deg"'), (T_BIAS, '<LogWavelengthDistribution minWavelength="20 micron" maxWavelength="30 micron"/>')], "Theta should be between 0 and pi."),
]


def refusal(tmp_path, fixture, edits):
    text = open(ski(fixture)).read()
    for old, new in edits:
        if hasattr(old, "subn"):
            text, count = old.subn(new, text, count=1)
        else:
            count = text.count(old) and 1
            text = text.replace(old, new, 1)
        assert count == 1, "the edit no longer applies to %s: %r" % (fixture, old)
    # (beside the fixture's input files: a variant that gets as far as reading one finds it)
    path = tmp_path / fixture
    path.write_text(text)
    try:
        Simulation(str(path)).setup()
    except RuntimeError as error:
        return str(error)
    return None


def ids(rows):
    return ["%d-%s" % (index, row[0][:-4]) for index, row in enumerate(rows)]


@pytest.mark.parametrize("fixture,edits,message", ROWS, ids=ids(ROWS))
def test_one_defect_is_refused_in_these_words(tmp_path, monkeypatch, fixture, edits, message):
    monkeypatch.setenv("SKH_INPUT_PATH", ski(""))
    assert refusal(tmp_path, fixture, edits) == message


@pytest.mark.parametrize("fixture,edits,message", ORDER, ids=ids(ORDER))
def test_of_two_defects_the_first_in_the_order_of_checks_is_named(tmp_path, monkeypatch, fixture, edits, message):
    monkeypatch.setenv("SKH_INPUT_PATH", ski(""))
    assert refusal(tmp_path, fixture, edits) == message


def test_a_missing_ski_file(tmp_path):
    path = str(tmp_path / "none.ski")
    with pytest.raises(RuntimeError) as refused:
        Simulation(path)
    assert str(refused.value) == "Cannot open ski file " + path
