"""Every header under voxmap_amd/csrc compiles when it is the only thing a unit
includes: the render kernel's stage headers (vx_math.h .. vx_pixel.h) name what
they use themselves, so no unit depends on the order it includes them in.  CPU
only: hipcc -fsyntax-only with the library's flags, no GPU, nothing linked."""
import os
import subprocess

import pytest

from voxmap_amd import build as vb

HEADERS = sorted(f for f in os.listdir(vb.CSRC) if f.endswith(".h"))


def test_build_lists_every_header():
    # an object is rebuilt when a header in build.HEADERS is newer: one that is missing there goes stale
    assert sorted(vb.HEADERS) == HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    unit = tmp_path / "only.hip"
    unit.write_text(f'#include "{header}"\n')
    r = subprocess.run([vb.hipcc(), *vb.FLAGS, f"-I{vb.CSRC}", "-fsyntax-only", str(unit)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
