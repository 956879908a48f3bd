"""Variants of the scenes under tests/ski that several test modules need: text replacements of a ski file, written to a directory of the
caller (tmp_path)."""
from conftest import ski

FIELD_GRID = ('<RadiationFieldOptions storeRadiationField="true"><radiationFieldWLG type="DisjointWavelengthGrid">%s</radiationFieldWLG>'
              "</RadiationFieldOptions>")
LOG_GRID = '<LogWavelengthGrid minWavelength="0.15 micron" maxWavelength="8 micron" numWavelengths="%d"/>'
ONE_BIN = '<ListWavelengthGrid wavelengths="1 micron" relativeHalfWidth="0.3" log="true"/>'


def with_field_grid(tmp_path, base, bins):
    """tests/ski/<base>.ski storing the radiation field on `bins` bins (a text replacement of its radiationFieldOptions)"""
    text = open(ski(base + ".ski")).read()
    a = text.index("<RadiationFieldOptions")
    b = text.index("</radiationFieldOptions>")
    text = text[:a] + FIELD_GRID % (ONE_BIN if bins == 1 else LOG_GRID % bins) + text[b:]
    path = tmp_path / f"{base}_{bins}.ski"
    path.write_text(text)
    return str(path)


def with_stored_field(tmp_path, base):
    """tests/ski/<base>.ski with storeRadiationField switched on (the scene's own radiation field grid)"""
    text = open(ski(base + ".ski")).read()
    assert text.count('storeRadiationField="false"') == 1
    path = tmp_path / f"{base}_rf.ski"
    path.write_text(text.replace('storeRadiationField="false"', 'storeRadiationField="true"'))
    return str(path)


def with_pixels(tmp_path, base, instrument, pixels):
    """tests/ski/<base>.ski with instrument `instrument` at pixels x pixels pixels"""
    lines = open(ski(base + ".ski")).read().split("\n")
    hits = [i for i, line in enumerate(lines) if f'instrumentName="{instrument}"' in line]
    assert len(hits) == 1
    line = lines[hits[0]]
    for axis in ("X", "Y"):
        a = line.index(f'numPixels{axis}="') + len(f'numPixels{axis}="')
        line = line[:a] + str(pixels) + line[line.index('"', a):]
    lines[hits[0]] = line
    path = tmp_path / f"{base}_{instrument}_{pixels}.ski"
    path.write_text("\n".join(lines))
    return str(path)


def with_optical_depth(tmp_path, base, depth):
    """tests/ski/<base>.ski with the optical depth of its (one) OpticalDepthMaterialNormalization set to `depth`: the same grid and density
    distribution, every density scaled"""
    import re
    text = open(ski(base + ".ski")).read()
    assert len(re.findall(r'<OpticalDepthMaterialNormalization [^>]*opticalDepth="[^"]*"', text)) == 1
    text = re.sub(r'(<OpticalDepthMaterialNormalization [^>]*opticalDepth=")[^"]*"', lambda m: f'{m.group(1)}{depth}"', text)
    path = tmp_path / f"{base}_tau{depth}.ski"
    path.write_text(text)
    return str(path)
